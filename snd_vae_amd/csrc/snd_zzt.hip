// Fused inner-product structure decoder + 2-class cross-entropy, fwd + bwd.
//
// Replaces, per graph: L = z z^T (InnerProductDecoder, layers.py:407-409),
// the diagonal rule (model.py:185,205-207), argmax (model.py:208), the
// accuracy count (main.py:334) and softmax_cross_entropy_with_logits
// (optimizer.py:142-144) plus its gradient.  The reference materialises
// [B,N,N,2] logits; here no logit ever reaches HBM.
//
// Split of the CE over pairs (i != j):  CE = softplus(L) - A L.
//   dense kernel (this file): sum_{i!=j} softplus(L_ij), #{L_ij > 0},
//                              dJd_i = sum_{j!=i} sigmoid(L_ij) z_j
//   edge kernel (snd_spmm.hip): the A-weighted terms over the CSR only.
// so the adjacency never enters the O(N^2 d) kernel.
//
// The dense kernel per (dtype, padded width dp = zzt_dp(d)); launch_zzt_dense picks it,
// each kernel's header comment below describes its structure:
//   bf16, dp = 32    zzt_dense_bf16_v4<32>  1024 threads, 32x32x16 MFMAs, signed epilogue
//   bf16, dp = 64    zzt_dense_bf16_v9      v4's per-wave work, two 512-thread workgroups per CU
//   bf16, dp = 128   zzt_dense_bf16_v7      v4's work split on one dual-use LDS image per tile
//   bf16, any dp     zzt_dense_bf16<dp>     v1, ZztArgs.variant 1 only (the bench's previous variant)
//   f32,  any dp     zzt_dense_f32<dp>      parity mode: v1's structure on the exact-f32 MFMA 16x16x4
// The bf16 defaults have a measurement instantiation each (MEAS, variant >= 256).
// Common to all: z is pre-scaled by sqrt(log2 e) for the K role (zzt_prep_kernel), so
// X = L log2(e) feeds v_exp_f32 (2^x) with no multiply.  Block -> (graph, row block) puts
// one graph's blocks on one XCD when B % 8 == 0 (blockIdx % 8 == graph % 8), so a graph's
// z stays in that XCD's L2.
#include "snd_zzt.hpp"

#include <type_traits>
#include "snd_spmm.hpp"

#include <algorithm>

namespace snd {
namespace {

constexpr int TJ = 64;      // columns per LDS tile
constexpr int ROWS = 128;   // rows per workgroup
constexpr int NTH = 512;

// row blocks a launch covers (ZztArgs.nrb; 0 = every row block of the graphs)
__host__ __device__ __forceinline__ int zrb(const ZztArgs& a) { return a.nrb ? a.nrb : a.npad / ROWS; }
// pairs (i, j) of row block rb with i or j a padding row: the mask-free kernels evaluate
// them as x = 0 (softplus2(0) = 1 each) and subtract them per row block
__device__ __forceinline__ double zzt_padded_pairs(const ZztArgs& a, int rb) {
  const int valid = max(0, min(ROWS, a.n - rb * ROWS));
  return (double)ROWS * a.npad - (double)valid * a.n;
}

// ---------------------------------------------------------------- prep
template <typename T, int DP>
__global__ void __launch_bounds__(256) zzt_prep_kernel(const float* z, int n, int npad,
                                                       int d, T* jrow, T* jt, float* colpart) {
  __shared__ float tile[64][DP + 1];
  __shared__ float stile[64][DP + 1];
  const int g = blockIdx.y, rb = blockIdx.x;
  const float sc = 1.2011224087864498f;  // sqrt(log2 e)
  for (int idx = threadIdx.x; idx < 64 * DP; idx += 256) {
    const int rr = idx / DP, c = idx - rr * DP;
    const int row = rb * 64 + rr;
    const float v = (row < n && c < d) ? z[((long long)g * n + row) * d + c] : 0.f;
    tile[rr][c] = v;
    const T b = (T)(v * sc);
    stile[rr][c] = (float)b;
    jrow[((long long)g * npad + row) * DP + c] = b;
  }
  __syncthreads();
  // per-64-row column sums of the stored (rounded) K-role values: sum_j x_ij
  // of every row i follows from them without touching the N^2 logits
  if (threadIdx.x < DP) {
    float cs = 0.f;
    for (int rr = 0; rr < 64; ++rr) cs += stile[rr][threadIdx.x];
    colpart[((long long)g * (npad / 64) + rb) * DP + threadIdx.x] = cs;
  }
  for (int idx = threadIdx.x; idx < 64 * DP; idx += 256) {
    const int c = idx >> 6, rr = idx & 63;
    jt[((long long)g * DP + c) * npad + rb * 64 + rr] = (T)tile[rr][c];
  }
}

// ---------------------------------------------------------------- epilogue
struct ChunkStats {
  double loss2;   // sum over valid pairs of max(x,0) + log2(1 + 2^-|x|), x = L log2 e
  unsigned cnt;   // #{x > 0}
};

// x[8]: logits (scaled) of this lane; j of element e = jbase + 16*(e>>2) + 4*q4 + (e&3)
template <bool SPECIAL>
__device__ __forceinline__ void chunk_epilogue(const float (&x)[8], float (&sv)[8],
                                               ChunkStats& st, int jbase, int q4,
                                               int i, int n) {
  float cs = 0.f, prod = 1.f;
  unsigned cnt = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bool valid = true;
    if constexpr (SPECIAL) {
      const int j = jbase + 16 * (e >> 2) + 4 * q4 + (e & 3);
      valid = (j < n) && (i < n) && (j != i);
    }
    const float xv = x[e];
    const float ex = __builtin_amdgcn_exp2f(-fabsf(xv));
    const float qd = 1.f + ex;
    const float rc = __builtin_amdgcn_rcpf(qd);
    const float sg = xv > 0.f ? rc : ex * rc;
    if (valid) {
      prod *= qd;
      cs += fmaxf(xv, 0.f);
      cnt += xv > 0.f ? 1u : 0u;
      sv[e] = sg;
    } else {
      sv[e] = 0.f;
    }
  }
  st.loss2 += (double)(cs + __builtin_amdgcn_logf(prod));
  st.cnt += cnt;
}

__device__ __forceinline__ void block_reduce_write(ChunkStats st, double* part) {
  __shared__ double sl[NTH / 64];
  __shared__ unsigned sc[NTH / 64];
  double l = wave_sum_d(st.loss2);
  unsigned c = wave_sum_u(st.cnt);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sl[w] = l; sc[w] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tl = 0.0, tc = 0.0;
    for (int k = 0; k < NTH / 64; ++k) { tl += sl[k]; tc += (double)sc[k]; }
    part[2 * blockIdx.x] = tl * (double)kLn2;
    part[2 * blockIdx.x + 1] = tc;
  }
}

// ---------------------------------------------------------------- bf16 MFMA, v1
// v1 (flash-style, no softmax normalisation needed; ZztArgs.variant 1):
//   workgroup = 8 waves x 16 rows i (128 rows of one graph); column tiles of
//   64 j staged in LDS twice -- z rows (K role) and z^T (V role) -- double
//   buffered, one barrier per tile.  Per 32-column chunk each wave runs
//   MFMA1  X[j,i] = z_j . z_i           (16x16x32 bf16, z_i held in VGPRs)
//   VALU   sigma / softplus / count on X (exp2 + rcp; one log2 per 8 logits
//          via the product identity sum log(1+e_k) = log prod(1+e_k))
//   MFMA2  dJd^T[c,i] += z^T[c,j] sigma[j,i]  -- the f32 accumulator X is
//          re-packed to bf16 in registers and used as the B operand directly
//          (no LDS round trip; k order permuted to match).
// LDS images are XOR-swizzled so the ds_read_b128 (K role) and ds_read_b64 (V role)
// operand reads are bank-conflict-free.
template <int DP> struct Swz;
template <> struct Swz<32> { static __device__ __forceinline__ int j(int) { return 0; } };
template <> struct Swz<64> { static __device__ __forceinline__ int j(int row) { return (row >> 1) & 7; } };
template <> struct Swz<128> { static __device__ __forceinline__ int j(int row) { return row & 15; } };
__device__ __forceinline__ int swz_t(int c) { return (c >> 1) & 7; }   // z^T image, 16 B chunks

template <int DP>
__global__ void __launch_bounds__(NTH) zzt_dense_bf16(ZztArgs a) {
  constexpr int JS = TJ * DP;          // z rows image (elements)
  constexpr int TS = DP * TJ;          // z^T image
  constexpr int KS = DP / 32;
  constexpr int CT = DP / 16;
  constexpr int CPR = DP / 8;          // 16 B chunks per z row
  constexpr int JCH = TJ * CPR, TCH = DP * (TJ / 8);
  constexpr int JPT = (JCH + NTH - 1) / NTH, TPT = (TCH + NTH - 1) / NTH;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2][JS + TS];

  const int g = blockIdx.x % a.ngraphs, rb = a.rb0 + blockIdx.x / a.ngraphs;
  const __bf16* Jg = reinterpret_cast<const __bf16*>(a.jrow) + (long long)g * a.npad * DP;
  const __bf16* JTg = reinterpret_cast<const __bf16*>(a.jt) + (long long)g * DP * a.npad;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, q4 = lane >> 4;
  const int i0 = rb * ROWS + 16 * w;

  bf16x8 bI[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    bI[ks] = *reinterpret_cast<const bf16x8*>(Jg + (long long)(i0 + r) * DP + 32 * ks + 8 * q4);
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 rj[JPT], rt[TPT];
  auto gload = [&](int t) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < JCH) {
        const int row = idx / CPR, ch = idx - row * CPR;
        rj[p] = *reinterpret_cast<const uint4*>(Jg + (long long)(t * TJ + row) * DP + ch * 8);
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < TCH) {
        const int c = idx >> 3, ch = idx & 7;
        rt[p] = *reinterpret_cast<const uint4*>(JTg + (long long)c * a.npad + t * TJ + ch * 8);
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < JCH) {
        const int row = idx / CPR, ch = idx - row * CPR;
        *reinterpret_cast<uint4*>(&lds[buf][row * DP + ((ch ^ Swz<DP>::j(row)) * 8)]) = rj[p];
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < TCH) {
        const int c = idx >> 3, ch = idx & 7;
        *reinterpret_cast<uint4*>(&lds[buf][JS + c * TJ + ((ch ^ swz_t(c)) * 8)]) = rt[p];
      }
    }
  };

  const int ntiles = a.npad / TJ;
  gload(0);
  sstore(0);
  __syncthreads();
  ChunkStats st{0.0, 0u};
  const int i_me = i0 + r;
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) gload(t + 1);
    const __bf16* Ls = lds[cur];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int jbase = t * TJ + 32 * q;
      f32x4 X0 = {0.f, 0.f, 0.f, 0.f}, X1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int ra = 32 * q + r, rb2 = 32 * q + 16 + r;
        const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
            &Ls[ra * DP + (((4 * ks + q4) ^ Swz<DP>::j(ra)) * 8)]);
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
            &Ls[rb2 * DP + (((4 * ks + q4) ^ Swz<DP>::j(rb2)) * 8)]);
        X0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bI[ks], X0, 0, 0, 0);
        X1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bI[ks], X1, 0, 0, 0);
      }
      float xs[8] = {X0[0], X0[1], X0[2], X0[3], X1[0], X1[1], X1[2], X1[3]};
      float sv[8];
      const bool special = (jbase + 32 > a.n) || (i0 + 16 > a.n) ||
                           (i0 >= jbase && i0 < jbase + 32);
      if (special) chunk_epilogue<true>(xs, sv, st, jbase, q4, i_me, a.n);
      else chunk_epilogue<false>(xs, sv, st, jbase, q4, i_me, a.n);
      bf16x8 sb;
#pragma unroll
      for (int e = 0; e < 8; ++e) sb[e] = (__bf16)sv[e];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = 16 * ct + r;
        const int u0 = 8 * q + q4, u1 = 8 * q + 4 + q4;     // 8 B units of 4 j
        const int sw = swz_t(c) << 1;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(&Ls[JS + c * TJ + ((u0 ^ sw) * 4)]);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(&Ls[JS + c * TJ + ((u1 ^ sw) * 4)]);
        const bf16x8 a2 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, sb, acc[ct], 0, 0, 0);
      }
    }
    if (t + 1 < ntiles) sstore(cur ^ 1);
    __syncthreads();
  }

  if (i_me < a.n) {
    float* dst = a.dJd + ((long long)g * a.n + i_me) * a.d;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c0 = 16 * ct + 4 * q4;
      if (c0 < a.d)
        *reinterpret_cast<float4*>(dst + c0) = make_float4(acc[ct][0], acc[ct][1], acc[ct][2], acc[ct][3]);
    }
  }
  block_reduce_write(st, a.part);
}

// ---------------------------------------------------------------- v4 / v7 geometry
// 1024-thread workgroup over 128 rows of one graph: 16 waves per CU (4 per SIMD)
// so one wave's VALU epilogue overlaps another's MFMAs; column tiles of TJ2 = 128.
// (Round 1's v2 and round 2's v3 -- 16x16x32 MFMAs, the |x| epilogue -- are retired.)
constexpr int TJ2 = 128;
constexpr int NTH2 = 1024;


// ---------------------------------------------------------------- f32 MFMA
// fp32 parity mode: v1's structure on the exact-f32 MFMA 16x16x4.
__device__ __forceinline__ int hJ(int row) { return ((row & 1) << 1) | (((row >> 1) & 7) << 2); }
__device__ __forceinline__ int hT(int c) { return (c & 3) | (((c >> 2) & 3) << 3); }

template <int DP>
__global__ void __launch_bounds__(NTH) zzt_dense_f32(ZztArgs a) {
  constexpr int JS = TJ * DP, TS = DP * TJ;
  constexpr int KS = DP / 4;
  constexpr int CT = DP / 16;
  constexpr int JCH = TJ * DP / 4, TCH = DP * TJ / 4;
  constexpr int JPT = (JCH + NTH - 1) / NTH, TPT = (TCH + NTH - 1) / NTH;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float* lds0 = dyn;
  float* lds1 = dyn + JS + TS;

  const int g = blockIdx.x % a.ngraphs, rb = a.rb0 + blockIdx.x / a.ngraphs;
  const float* Jg = reinterpret_cast<const float*>(a.jrow) + (long long)g * a.npad * DP;
  const float* JTg = reinterpret_cast<const float*>(a.jt) + (long long)g * DP * a.npad;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, q4 = lane >> 4;
  const int i0 = rb * ROWS + 16 * w;

  float bI[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bI[ks] = Jg[(long long)(i0 + r) * DP + 4 * ks + q4];
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 rj[JPT], rt[TPT];
  auto gload = [&](int t) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < JCH) {
        const int row = idx / (DP / 4), c4 = idx - row * (DP / 4);
        rj[p] = *reinterpret_cast<const float4*>(Jg + (long long)(t * TJ + row) * DP + 4 * c4);
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < TCH) {
        const int c = idx >> 4, c4 = idx & 15;
        rt[p] = *reinterpret_cast<const float4*>(JTg + (long long)c * a.npad + t * TJ + 4 * c4);
      }
    }
  };
  auto sstore = [&](float* L) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < JCH) {
        const int row = idx / (DP / 4), c4 = idx - row * (DP / 4);
        const int h = hJ(row);
        const float v[4] = {rj[p].x, rj[p].y, rj[p].z, rj[p].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) L[row * DP + ((4 * c4 + e) ^ h)] = v[e];
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NTH;
      if (idx < TCH) {
        const int c = idx >> 4, c4 = idx & 15;
        const int h = hT(c);
        const float v[4] = {rt[p].x, rt[p].y, rt[p].z, rt[p].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) L[JS + c * TJ + ((4 * c4 + e) ^ h)] = v[e];
      }
    }
  };

  const int ntiles = a.npad / TJ;
  gload(0);
  sstore(lds0);
  __syncthreads();
  ChunkStats st{0.0, 0u};
  const int i_me = i0 + r;
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) gload(t + 1);
    const float* Ls = cur ? lds1 : lds0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int jbase = t * TJ + 32 * q;
      f32x4 X0 = {0.f, 0.f, 0.f, 0.f}, X1 = {0.f, 0.f, 0.f, 0.f};
      const int ra = 32 * q + r, rb2 = 32 * q + 16 + r;
      const int ha = hJ(ra), hb = hJ(rb2);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const float a0 = Ls[ra * DP + ((4 * ks + q4) ^ ha)];
        const float a1 = Ls[rb2 * DP + ((4 * ks + q4) ^ hb)];
        X0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bI[ks], X0, 0, 0, 0);
        X1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bI[ks], X1, 0, 0, 0);
      }
      float xs[8] = {X0[0], X0[1], X0[2], X0[3], X1[0], X1[1], X1[2], X1[3]};
      float sv[8];
      const bool special = (jbase + 32 > a.n) || (i0 + 16 > a.n) ||
                           (i0 >= jbase && i0 < jbase + 32);
      if (special) chunk_epilogue<true>(xs, sv, st, jbase, q4, i_me, a.n);
      else chunk_epilogue<false>(xs, sv, st, jbase, q4, i_me, a.n);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = 16 * ct + r;
        const int h = hT(c);
        const float* row = Ls + JS + c * TJ;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[(32 * q + 4 * q4 + rr) ^ h], sv[rr],
                                                         acc[ct], 0, 0, 0);
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[(32 * q + 16 + 4 * q4 + rr) ^ h],
                                                         sv[4 + rr], acc[ct], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntiles) sstore(cur ? lds0 : lds1);
    __syncthreads();
  }

  if (i_me < a.n) {
    float* dst = a.dJd + ((long long)g * a.n + i_me) * a.d;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c0 = 16 * ct + 4 * q4;
      if (c0 < a.d)
        *reinterpret_cast<float4*>(dst + c0) = make_float4(acc[ct][0], acc[ct][1], acc[ct][2], acc[ct][3]);
    }
  }
  block_reduce_write(st, a.part);
}

// ---------------------------------------------------------------- bf16 MFMA, v4
// v4: v_mfma_f32_32x32x16_bf16, a select-free epilogue, software-pipelined tiles.
//
// Work split.  1024-thread workgroup = 4 row groups (32 rows i) x 4 column
// blocks (32 j of every 128-column tile): each wave owns one 32 x 32 logit
// block per tile.  A 32x32x16 MFMA holds the SIMD's vector issue for 8 of its
// 32 cycles (16x16x32: 8 of 16), and a block needs half v3's LDS operand reads.
//   fwd   Y[j][i] = -x_ij            A = z_j rows (LDS tile), B = -z_i (LDS image
//                                    of the workgroup's rows, negated; registers
//                                    are the scarce resource at 4 waves per SIMD)
//   bwd   dJ'[i][c] += S'[i][j] z_j[c] A = S' packed straight from Y's registers
//                                    (its column i is on the lane), B = z^T
//                                    (LDS, j order permuted to match)
// Epilogue per logit, y = -x:
//   e = 2^y; q = 1 + e; s = 1/q = sigmoid(x); per QUAD of logits one
//   log2(q_a q_b q_c q_d); #{x > 0} = #{sign(y)}: sign bytes of 4 logits gathered by two
//   v_perm and popcounted (1 op per logit instead of a compare + SALU ballot).
// softplus2(x) = x + log2(q) with sum_j x_ij = z_i . colsum (analytic): no |x|
// and no select per logit.  sigmoid(x) = 1 / (1 + 2^-x) is exact and finite for
// every x (q = inf -> 0).  A quad product overflows only when x_a + .. + x_d < -128
// (L_a + .. + L_d < -88.7): that lane recomputes the block's loss terms in the |x|
// form (one wave-uniform test per block when nothing overflows).
// Measured rates (tools/micro/valu_rate.hip, 4 waves per SIMD): a transcendental
// costs ~3.4 FMAs of issue and does not co-issue with them.  This signed epilogue
// (2.25 transcendentals + ~2.5 other ops per logit) beat round 1's |x| form
// (2.125 + ~6.9).  Tiles are triple-buffered (global loads two tiles ahead).
// Variants measured slower and retired: the next tile's forward MFMAs
// before this tile's epilogue (spills at d = 64), odd column blocks' backward one
// tile late, the |x| epilogue, one wave per SIMD with a block-level software
// pipeline (v8: 89-95 us against 60 us).
// LDS images carry one 16 B pad per row: every operand read of a lane group
// lands on 16 distinct 4-bank groups and all k-steps / output blocks of a lane
// share one address register.  The diagonal correction reads z_i[c] from a
// transposed LDS copy of the workgroup's z^T columns (one coalesced load).

template <int DP, bool MEAS>
__global__ void __launch_bounds__(NTH2) zzt_dense_bf16_v4(ZztArgs a) {
  constexpr int NT = NTH2, NW = NT / 64;
  constexpr int KS = DP / 16;          // forward k-steps
  constexpr int CB = DP / 32;          // backward 32-column output blocks
  constexpr int JST = DP + 8;          // J / row image stride (elements)
  constexpr int TST = TJ2 + 8;         // z^T image stride
  constexpr int JS = TJ2 * JST;
  constexpr int TS = DP * TST;
  constexpr int BUF = JS + TS;
  constexpr int CPR = DP / 8, TCPR = TJ2 / 8;
  constexpr int JCH = TJ2 * CPR, TCH = DP * TCPR;
  constexpr int JPT = (JCH + NT - 1) / NT, TPT = (TCH + NT - 1) / NT;
  constexpr unsigned NEG = 0x80008000u;   // B operand sign: the forward computes y = -x
  __shared__ __attribute__((aligned(16))) __bf16 lds[3 * BUF];
  __shared__ __attribute__((aligned(16))) __bf16 brows[ROWS * JST];   // (-)z_i rows (scaled)
  __shared__ __attribute__((aligned(16))) __bf16 zown[ROWS * JST];    // z_i rows (z^T values)
  __shared__ float colsum[DP];
  __shared__ float csred[NT / DP][DP];
  __shared__ float dsg[4][32];         // per row group: s'_ii (bf16-rounded)
  __shared__ double sl[NW];
  __shared__ unsigned sc[NW];

  // measurement only (MEAS builds, variant >> 8): phase-skip bits 1 epilogue,
  // 2 forward MFMAs, 4 backward MFMAs, 8 tile staging, 16 the tile loop, 64 the
  // tile barrier (with 8); 32 s_memrealtime stamps over part[] (results wrong);
  // 128 (with 32) the tile loop's shader-clock cycles instead (tools/zzt_stamps.py)
  const int skip = MEAS ? __builtin_amdgcn_readfirstlane(a.variant >> 8) : 0;
  unsigned long long ts[4] = {0, 0, 0, 0};
  if (skip & 32) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int wgs = a.ngraphs * zrb(a);
  const int sp = blockIdx.x / wgs, bx = blockIdx.x - sp * wgs;
  const int nsplit = gridDim.x / wgs;
  const int g = bx % a.ngraphs, rb = a.rb0 + bx / a.ngraphs;
  const __bf16* Jg = reinterpret_cast<const __bf16*>(a.jrow) + (long long)g * a.npad * DP;
  const __bf16* JTg = reinterpret_cast<const __bf16*>(a.jt) + (long long)g * DP * a.npad;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int rg = w & 3, cb = w >> 2;
  const int i0 = __builtin_amdgcn_readfirstlane(rb * ROWS + 32 * rg);
  const int i_me = i0 + r;
  const int ntot = a.npad / TJ2;
  const int t0 = sp * ntot / nsplit, t1 = (sp + 1) * ntot / nsplit;

  uint4 rj[JPT], rt[TPT];
  auto gload = [&](int t) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NT;
      if (JCH % NT == 0 || idx < JCH) {
        const int row = idx / CPR, ch = idx - row * CPR;
        rj[p] = *reinterpret_cast<const uint4*>(Jg + (long long)(t * TJ2 + row) * DP + ch * 8);
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NT;
      if (TCH % NT == 0 || idx < TCH) {
        const int c = idx / TCPR, ch = idx - c * TCPR;
        rt[p] = *reinterpret_cast<const uint4*>(JTg + (long long)c * a.npad + t * TJ2 + ch * 8);
      }
    }
  };
  // J rows: [row][k].  z^T: row c holds, per 32-j block jb and k-step s, chunk
  // 4 jb + 2 s + h = {j = 32 jb + 16 s + 4 h + 0..3, + 8 + 0..3} (the k order of
  // the packed S' operand).
  auto sstore = [&](__bf16* L) {
#pragma unroll
    for (int p = 0; p < JPT; ++p) {
      const int idx = tid + p * NT;
      if (JCH % NT == 0 || idx < JCH) {
        const int row = idx / CPR, ch = idx - row * CPR;
        *reinterpret_cast<uint4*>(&L[row * JST + ch * 8]) = rj[p];
      }
    }
#pragma unroll
    for (int p = 0; p < TPT; ++p) {
      const int idx = tid + p * NT;
      if (TCH % NT == 0 || idx < TCH) {
        const int c = idx / TCPR, ch = idx - c * TCPR;
        const int jb = ch >> 2, m = ch & 3, s = m >> 1, a8 = (m & 1) * 4;
        __bf16* row = &L[JS + c * TST + (4 * jb + 2 * s) * 8 + a8];
        *reinterpret_cast<uint2*>(row) = make_uint2(rt[p].x, rt[p].y);
        *reinterpret_cast<uint2*>(row + 8) = make_uint2(rt[p].z, rt[p].w);
      }
    }
  };

  // ---- prologue: first tile in flight, then the workgroup's own rows, z^T
  // columns and the graph column sums
  gload(t0);
  for (int idx = tid; idx < ROWS * CPR; idx += NT) {
    const int row = idx / CPR, ch = idx - row * CPR;
    const uint4 u = *reinterpret_cast<const uint4*>(Jg + (long long)(rb * ROWS + row) * DP + ch * 8);
    *reinterpret_cast<uint4*>(&brows[row * JST + ch * 8]) =
        make_uint4(u.x ^ NEG, u.y ^ NEG, u.z ^ NEG, u.w ^ NEG);
  }
  for (int idx = tid; idx < DP * (ROWS / 8); idx += NT) {   // z^T[c][rb*128 + 8u ..] -> zown[i][c]
    const int c = idx / (ROWS / 8), u = idx - c * (ROWS / 8);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(JTg + (long long)c * a.npad + rb * ROWS + 8 * u);
#pragma unroll
    for (int e = 0; e < 8; ++e) zown[(8 * u + e) * JST + c] = v[e];
  }
  {   // graph column sums S_k = sum_j zs_jk (fixed order over the 64-row partials)
    const int nrb = a.npad / 64;
    const int k = tid % DP, grp = tid / DP;
    float s = 0.f;
    for (int p = grp; p < nrb; p += NT / DP) s += a.colpart[((long long)g * nrb + p) * DP + k];
    csred[grp][k] = s;
  }
  sstore(lds);
  gload(min(t0 + 1, t1 - 1));
  sstore(lds + BUF);
  __syncthreads();
  if (tid < DP) {
    float s = 0.f;
    for (int p = 0; p < NT / DP; ++p) s += csred[p][tid];
    colsum[tid] = s;
  }
  unsigned long long tcy[2] = {0, 0};   // shader-clock cycles (s_memtime) over the tile loop
  if (skip & 32) { ts[1] = __builtin_amdgcn_s_memrealtime(); tcy[0] = __builtin_amdgcn_s_memtime(); }

  f32x16 cinit, acc[CB];
  // +0 accumulator init: a zero accumulator folds into the MFMA's inline constant 0 (a
  // -0.0 splat pinned 16 VGPRs and cost 24 moves per tile)
#pragma unroll
  for (int v = 0; v < 16; ++v) cinit[v] = 0.f;
#pragma unroll
  for (int q = 0; q < CB; ++q)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[q][v] = 0.f;
  auto fwd = [&](const __bf16* L) {
    f32x16 X = cinit;
    const int j = 32 * cb + r;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(&L[j * JST + (2 * s + h) * 8]);
      const bf16x8 bv = *reinterpret_cast<const bf16x8*>(&brows[(32 * rg + r) * JST + (2 * s + h) * 8]);
      X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, X, 0, 0, 0);
    }
    return X;
  };
  float lacc = 0.f;
  double ltot = 0.0;
  unsigned lcnt = 0;   // per lane: sign bits counted
  // sticky, wave-uniform: once a quad product of this wave overflowed, later tiles skip
  // the products (logits that large, e.g. C4's graph-latent heads at init, recur)
  bool ovf = false;
  auto epi = [&](const f32x16& Y, bf16x8 (&sA)[2]) {
    float q[16], lt = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float e = __builtin_amdgcn_exp2f(Y[v]);
      q[v] = e + 1.f;
      sA[v >> 3][v & 7] = (__bf16)__builtin_amdgcn_rcpf(q[v]);
    }
    // #{x > 0} = #{y < 0} (y = +0 where x = 0): the sign bytes of four y's gathered
    // by two v_perm, masked, popcounted into a per-lane count
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const unsigned t01 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 1]),
                                                 __float_as_uint(Y[4 * g4]), 0x0C0C0703u);
      const unsigned t23 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 3]),
                                                 __float_as_uint(Y[4 * g4 + 2]), 0x07030C0Cu);
      lcnt += (unsigned)__builtin_popcount((t01 | t23) & 0x80808080u);
    }
    if (!ovf) {
#pragma unroll
      for (int p = 0; p < 4; ++p)   // one log2 per 4 logits (an overflowing product: fallback below)
        lt += __builtin_amdgcn_logf((q[4 * p] * q[4 * p + 1]) * (q[4 * p + 2] * q[4 * p + 3]));
      ovf = __builtin_amdgcn_ballot_w64(!__builtin_isfinite(lt)) != 0;
    }
    if (__builtin_expect(ovf, 0)) {
      // a quad product overflowed: the block one logit at a time,
      // log2(q) = y for y > 24 (1 + 2^y rounds to 2^y; q may be inf), else log2(q)
      // (one transcendental per logit on the q already computed)
      lt = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) lt += Y[v] > 24.f ? Y[v] : __builtin_amdgcn_logf(q[v]);
    }
    lacc += lt;
  };
  auto bwd = [&](const __bf16* L, const bf16x8 (&sA)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < CB; ++q) {
        const int c = 32 * q + r;
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(&L[JS + c * TST + (4 * cb + 2 * s + h) * 8]);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sA[s], bv, acc[q], 0, 0, 0);
      }
  };

  f32x16 Y;
  // one tile; buffer indices are compile-time, the last tiles re-stage the final
  // tile (branch-free body)
  auto tile = [&](int t, auto cc) {
    constexpr int CUR = decltype(cc)::value, NN = (CUR + 2) % 3;
    if (!(skip & 8)) gload(min(t + 2, t1 - 1));
    Y = (skip & 2) ? cinit : fwd(lds + CUR * BUF);
    bf16x8 sA[2];
    if (skip & 1) {
#pragma unroll
      for (int v = 0; v < 16; ++v) sA[v >> 3][v & 7] = (__bf16)Y[v];
    } else {
      epi(Y, sA);
    }
    if (!(skip & 4)) bwd(lds + CUR * BUF, sA);
    else lacc += (float)sA[0][0];
    if (!(skip & 8)) sstore(lds + NN * BUF);
    if (!(skip & 64)) __syncthreads();
  };
  const int tl1 = (skip & 16) ? t0 : t1;
  for (int t = t0; t < tl1; t += 3) {
    tile(t, std::integral_constant<int, 0>{});
    if (t + 1 < tl1) tile(t + 1, std::integral_constant<int, 1>{});
    if (t + 2 < tl1) tile(t + 2, std::integral_constant<int, 2>{});
    ltot += (double)lacc;   // keep the fp32 partial sums short
    lacc = 0.f;
  }
  if (skip & 32) { ts[2] = __builtin_amdgcn_s_memrealtime(); tcy[1] = __builtin_amdgcn_s_memtime(); }

  // ---- per-row corrections (row i_me; lanes r and r + 32 hold its two k halves)
  float xd = 0.f, xs = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(&brows[(32 * rg + r) * JST + 16 * s + 8 * h]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float bb = (float)bv[e];   // (-)z_i: the products below do not see the sign
      xd += bb * bb;
      xs += bb * colsum[16 * s + 8 * h + e];
    }
  }
  xd += __shfl_xor(xd, 32, 64);
  xs += __shfl_xor(xs, 32, 64);
  xs = -xs;
  const bool row_valid = i_me < a.n;
  const bool corr = sp == 0;
  const bool own = cb == 0 && h == 0 && row_valid && corr;
  const float exd = __builtin_amdgcn_exp2f(-fabsf(xd));
  if (own) {   // + sum_j x_ij (softplus2(x) = x + log2(q)), - softplus2(x_ii)
    ltot += (double)xs;
    ltot -= (double)(fmaxf(xd, 0.f) + __builtin_amdgcn_logf(1.f + exd));
  }
  const unsigned dpos = (unsigned)__popcll(__ballot(own && xd > 0.f));
  if (cb == 0 && h == 0) {   // s'_ii as the backward MFMA consumed it (bf16), 0 outside split 0
    const float sg = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(-xd) + 1.f);
    dsg[rg][r] = corr ? (float)(__bf16)sg : 0.f;
  }

  // ---- combine the four column blocks' partial dJ' (fixed order) through LDS
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);   // [cb-1][rg][CB*16][64]
  if (cb > 0) {
#pragma unroll
    for (int q = 0; q < CB; ++q)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        red[(((cb - 1) * 4 + rg) * (CB * 16) + q * 16 + v) * 64 + lane] = acc[q][v];
  }
  __syncthreads();
  if (cb == 0 && !(skip & 32)) {
    float* dst = (sp == 0 ? a.dJd : a.dJd_extra + (long long)(sp - 1) * a.ngraphs * a.n * a.d) +
                 (long long)g * a.n * a.d;
#pragma unroll
    for (int q = 0; q < CB; ++q) {
      const int c = 32 * q + r;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float o = acc[q][v];
#pragma unroll
        for (int k = 0; k < 3; ++k) o += red[((k * 4 + rg) * (CB * 16) + q * 16 + v) * 64 + lane];
        const int il = (v & 3) + 8 * (v >> 2) + 4 * h;   // D row within the row group
        const int i = i0 + il;
        if (i < a.n && c < a.d)
          dst[(long long)i * a.d + c] = o - dsg[rg][il] * (float)zown[(32 * rg + il) * JST + c];
      }
    }
  }
  const double l = wave_sum_d(ltot);
  const unsigned wcnt = wave_sum_u(lcnt);
  if (lane == 0) { sl[w] = l; sc[w] = wcnt - dpos; }
  __syncthreads();
  if (tid == 0) {
    double tl = 0.0, tc = 0.0;
    for (int k = 0; k < NW; ++k) { tl += sl[k]; tc += (double)sc[k]; }
    if (corr)   // padded pairs of this row block: x = 0 exactly, softplus2(0) = 1 each
      tl -= zzt_padded_pairs(a, rb);
    a.part[2 * blockIdx.x] = tl * (double)kLn2;
    a.part[2 * blockIdx.x + 1] = tc;
    if (skip & 32) {
      ts[3] = __builtin_amdgcn_s_memrealtime();
      unsigned* o = reinterpret_cast<unsigned*>(a.part + 2 * blockIdx.x);
      for (int k = 0; k < 4; ++k) o[k] = (unsigned)ts[k];
      if (skip & 128) {   // tile loop: 100 MHz stamps and shader-clock cycles instead
        o[0] = (unsigned)ts[1]; o[1] = (unsigned)ts[2]; o[2] = (unsigned)tcy[0]; o[3] = (unsigned)tcy[1];
      }
    }
  }
}

// ---------------------------------------------------------------- bf16 MFMA, v7 (d = 128)
// v4's work split and signed epilogue at d = 128, where v4's two LDS images
// per tile (z rows and z^T, 2 x 35 KB) cannot be triple-buffered beside the
// workgroup's own rows.  One image per tile serves both products:
//   * layout: 8-row x 32-column subtiles of 512 B, 16-byte chunks XOR-swizzled
//     (zoa; MI355X guide T10 "one image for row reads AND transposed reads"): the
//     forward A operand (z_j rows) is a ds_read_b128 row read, the backward B operand
//     (z_j[c] for the 8 j of a k-slot, column c on the lane) two ds_read_b64_tr_b16
//     transposed reads of the same image; both conflict-free, 2 address bases each;
//   * the image holds z * sqrt(log2 e) (the forward's scaled rows), so the backward
//     sums scaled z_j and the result is divided by sqrt(log2 e) once at the end
//     (within bf16 rounding of v3's unscaled z^T operand);
//   * tiles arrive by LDS-DMA (asm-issued, counted vmcnt) into a 3-deep ring, the
//     workgroup's -z_i rows sit in a fourth image: 128 KB of LDS;
//   * the four column blocks' partial dJ are combined through LDS in two passes
//     (two 32-column output blocks each: 98 KB).
// Per wave and tile: 8 forward + 8 backward v_mfma_f32_32x32x16_bf16, the same
// epilogue VALU as v4 at d = 64: twice v4's MFMA work per logit.
typedef short zv4s __attribute__((ext_vector_type(4)));
typedef short zv8s __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) zv4s zlds_v4s;
typedef __attribute__((address_space(3))) void* zlptr_t;

__device__ __forceinline__ int zoa(int row, int ch) {   // byte offset of (row, 16-byte chunk ch)
  return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}
// one 16-byte LDS-DMA per lane to the wave-uniform LDS byte address dst + 16 lane,
// issued from inline asm: the compiler neither tracks nor drains it
__device__ __forceinline__ void zdma16(const void* g, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
               "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
}
__device__ __forceinline__ bf16x8 ztr_pair(const char* p0, const char* p1) {
  const zv4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((zlds_v4s*)(p0));
  const zv4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((zlds_v4s*)(p1));
  const zv8s c = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}
constexpr float kInvSqrtLog2e = 0.8325546111576977f;   // 1 / sqrt(log2 e)

template <bool MEAS>
__global__ void __launch_bounds__(NTH2) zzt_dense_bf16_v7(ZztArgs a) {
  constexpr int DP = 128, NT = NTH2, NW = NT / 64;
  constexpr int KS = DP / 16;          // forward k-steps
  constexpr int CB = DP / 32;          // backward 32-column output blocks
  constexpr int IMG = TJ2 * DP * 2;    // one [128][128] bf16 image, 32 KB
  __shared__ __attribute__((aligned(16))) char lds[4 * IMG];   // 3 tile buffers, -z_i rows
  __shared__ float colsum[DP];
  __shared__ float csred[NT / DP][DP];
  __shared__ float dsg[4][32];
  __shared__ double sl[NW];
  __shared__ unsigned sc[NW];
  char* brows = lds + 3 * IMG;
  const unsigned lds0 = (unsigned)(uintptr_t)(zlptr_t)lds;

  // measurement only (MEAS, variant >> 8): 1 skips the epilogue, 2 the forward MFMAs,
  // 4 the backward MFMAs, 8 the tile DMAs (results wrong)
  const int skip = MEAS ? __builtin_amdgcn_readfirstlane(a.variant >> 8) : 0;
  const int wgs = a.ngraphs * zrb(a);
  const int sp = blockIdx.x / wgs, bx = blockIdx.x - sp * wgs;
  const int nsplit = gridDim.x / wgs;
  const int g = bx % a.ngraphs, rb = a.rb0 + bx / a.ngraphs;
  const __bf16* Jg = reinterpret_cast<const __bf16*>(a.jrow) + (long long)g * a.npad * DP;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int rg = w & 3, cb = w >> 2;
  const int i0 = __builtin_amdgcn_readfirstlane(rb * ROWS + 32 * rg);
  const int i_me = i0 + r;
  const int ntot = a.npad / TJ2;
  const int t0 = sp * ntot / nsplit, t1 = (sp + 1) * ntot / nsplit;

  // tile t -> ring buffer b: 32 pieces of 1 KB, wave w issues pieces w and w + 16.
  // Piece P, lane l lands at 1024 P + 16 l = row 8 (P >> 1) + ((l >> 2) & 7), chunk
  // 4 (2 (P & 1) + (l >> 5)) + ((l & 3) ^ ((row >> 2) & 3)) of the image (zoa inverse)
  int dsrc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int P = w + 16 * k;
    const int row = 8 * (P >> 1) + ((lane >> 2) & 7);
    const int ch = 4 * (2 * (P & 1) + (lane >> 5)) + ((lane & 3) ^ ((row >> 2) & 3));
    dsrc[k] = row * DP + 8 * ch;
  }
  auto dma = [&](int t, int b) {
    if (MEAS && (skip & 8)) return;
#pragma unroll
    for (int k = 0; k < 2; ++k)
      zdma16(Jg + (long long)t * TJ2 * DP + dsrc[k],
             __builtin_amdgcn_readfirstlane(lds0 + b * IMG + 1024 * (w + 16 * k)));
  };

  // ---- prologue: tile t0 in flight; -z_i rows; column sums
  dma(t0, 0);
  for (int idx = tid; idx < ROWS * (DP / 8); idx += NT) {
    const int row = idx >> 4, ch = idx & 15;
    const uint4 u = *reinterpret_cast<const uint4*>(Jg + (long long)(rb * ROWS + row) * DP + ch * 8);
    *reinterpret_cast<uint4*>(brows + zoa(row, ch)) =
        make_uint4(u.x ^ 0x80008000u, u.y ^ 0x80008000u, u.z ^ 0x80008000u, u.w ^ 0x80008000u);
  }
  {
    const int nrb = a.npad / 64;
    const int k = tid % DP, grp = tid / DP;
    float s = 0.f;
    for (int p = grp; p < nrb; p += NT / DP) s += a.colpart[((long long)g * nrb + p) * DP + k];
    csred[grp][k] = s;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < DP) {
    float s = 0.f;
    for (int p = 0; p < NT / DP; ++p) s += csred[p][tid];
    colsum[tid] = s;
  }

  f32x16 acc[CB];
#pragma unroll
  for (int q = 0; q < CB; ++q)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[q][v] = 0.f;
  // forward operand bases (k-step s: base[s & 1] + 512 (s >> 1))
  const int ja = 32 * cb + r, ia = 32 * rg + r;
  const int fa0 = zoa(ja, h), fa1 = zoa(ja, 2 + h);
  const int fb0 = zoa(ia, h), fb1 = zoa(ia, 2 + h);
  // backward transposed-read bases: lane 4 qq + pp of group gq supplies row
  // 32 cb + 16 s + 8 t + 4 (gq >> 1) + qq, columns 32 q + 16 (gq & 1) + 4 pp .. + 3
  const int gq = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
  const int c0 = 2 * (gq & 1) + (pp >> 1);
  const int tb0 = 2048 * (4 * cb) + 64 * (4 * (gq >> 1) + qq) + 16 * (c0 ^ (gq >> 1)) + 8 * (pp & 1);
  const int tb1 = 2048 * (4 * cb + 1) + 64 * (4 * (gq >> 1) + qq) + 16 * (c0 ^ ((gq >> 1) + 2)) + 8 * (pp & 1);
  auto fwd = [&](int b) {
    f32x16 X;
#pragma unroll
    for (int v = 0; v < 16; ++v) X[v] = 0.f;
    if (MEAS && (skip & 2)) return X;
    const char* T = lds + b * IMG;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(T + ((s & 1) ? fa1 : fa0) + 512 * (s >> 1));
      const bf16x8 bv = *reinterpret_cast<const bf16x8*>(brows + ((s & 1) ? fb1 : fb0) + 512 * (s >> 1));
      X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, X, 0, 0, 0);
    }
    return X;
  };
  float lacc = 0.f;
  double ltot = 0.0;
  unsigned lcnt = 0;
  auto epi = [&](const f32x16& Y, bf16x8 (&sA)[2]) {   // v4's epilogue, y = -x
    if (MEAS && (skip & 1)) {
#pragma unroll
      for (int v = 0; v < 16; ++v) sA[v >> 3][v & 7] = (__bf16)Y[v];
      return;
    }
    float q[16], lt = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float e = __builtin_amdgcn_exp2f(Y[v]);
      q[v] = e + 1.f;
      sA[v >> 3][v & 7] = (__bf16)__builtin_amdgcn_rcpf(q[v]);
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const unsigned t01 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 1]),
                                                 __float_as_uint(Y[4 * g4]), 0x0C0C0703u);
      const unsigned t23 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 3]),
                                                 __float_as_uint(Y[4 * g4 + 2]), 0x07030C0Cu);
      lcnt += (unsigned)__builtin_popcount((t01 | t23) & 0x80808080u);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
      lt += __builtin_amdgcn_logf((q[4 * p] * q[4 * p + 1]) * (q[4 * p + 2] * q[4 * p + 3]));
    if (__builtin_expect(!__builtin_isfinite(lt), 0)) {   // a quad product overflowed
      lt = 0.f;   // log2(q) per logit: y past 24 exactly, else log2 of the q already computed
#pragma unroll
      for (int v = 0; v < 16; ++v) lt += Y[v] > 24.f ? Y[v] : __builtin_amdgcn_logf(q[v]);
    }
    lacc += lt;
  };
  auto bwd = [&](int b, const bf16x8 (&sA)[2]) {
    if (MEAS && (skip & 4)) { lacc += (float)sA[0][0]; return; }
    const char* T = lds + b * IMG;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < CB; ++q) {
        const bf16x8 bv = ztr_pair(T + tb0 + 4096 * s + 512 * q, T + tb1 + 4096 * s + 512 * q);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sA[s], bv, acc[q], 0, 0, 0);
      }
  };

  // tile t in ring slot CUR: DMA of tile t+2 into the slot tile t-1 left, forward,
  // epilogue, backward; wait for tile t+1 (its 2 DMAs per wave; t+2's may fly), barrier.
  // Stagger: the odd column-block waves (two of the four waves of every SIMD: waves w and
  // w + 4k share one) run one tile late -- tile t-1's epilogue and backward, then tile
  // t's forward -- so after every barrier half of each SIMD's waves start on the VALU
  // while the other half starts on the matrix pipe (the phases otherwise serialise:
  // all four waves open a tile with their forward MFMAs and close it with the
  // backward ones).  Three slots hold tiles t-1 (late backward), t and t+1 (DMA'd
  // one tile ahead into the slot of tile t-2).
  // (the two roles run separate loops, so the early waves do not keep the late waves'
  // carried logits live)
  auto run = [&](auto late_c) {
    constexpr bool LATE = decltype(late_c)::value;
    f32x16 Yp;
#pragma unroll
    for (int v = 0; v < 16; ++v) Yp[v] = 0.f;
    auto tile = [&](int t, auto cc) {
      constexpr int CUR = decltype(cc)::value, NN = (CUR + 2) % 3;
      if (t + 1 < t1) dma(t + 1, (CUR + 1) % 3);
      if constexpr (LATE) {
        if (t > t0) {
          bf16x8 sA[2];
          epi(Yp, sA);
          bwd(NN, sA);   // tile t-1's slot
        }
        Yp = fwd(CUR);
      } else if (!(MEAS && (skip & 16) && (t & 1))) {
        const f32x16 Y = fwd(CUR);
        bf16x8 sA[2];
        epi(Y, sA);
        bwd(CUR, sA);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t+1 landed
      __syncthreads();
    };
    for (int t = t0; t < t1; t += 3) {
      tile(t, std::integral_constant<int, 0>{});
      if (t + 1 < t1) tile(t + 1, std::integral_constant<int, 1>{});
      if (t + 2 < t1) tile(t + 2, std::integral_constant<int, 2>{});
      ltot += (double)lacc;
      lacc = 0.f;
    }
    if (LATE && t1 > t0) {   // the late waves' last tile (its slot is intact: no DMA after the loop)
      bf16x8 sA[2];
      epi(Yp, sA);
      bwd((t1 - 1 - t0) % 3, sA);
      ltot += (double)lacc;
      lacc = 0.f;
    }
  };
  // static priority 1 for the late waves (MI355X guide, two waves per SIMD item 4):
  // 324 vs 330 us at 2 graphs; priority 1 for the early waves instead 331
  if (cb & 1) {
    __builtin_amdgcn_s_setprio(1);
    run(std::true_type{});
    __builtin_amdgcn_s_setprio(0);
  } else {
    run(std::false_type{});
  }

  // ---- per-row corrections (row i_me; lanes r and r + 32 hold its two k halves)
  float xd = 0.f, xs = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(brows + ((s & 1) ? fb1 : fb0) + 512 * (s >> 1));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float bb = (float)bv[e];
      xd += bb * bb;
      xs += bb * colsum[16 * s + 8 * h + e];
    }
  }
  xd += __shfl_xor(xd, 32, 64);
  xs += __shfl_xor(xs, 32, 64);
  xs = -xs;
  const bool row_valid = i_me < a.n;
  const bool corr = sp == 0;
  const bool own = cb == 0 && h == 0 && row_valid && corr;
  const float exd = __builtin_amdgcn_exp2f(-fabsf(xd));
  if (own) {
    ltot += (double)xs;
    ltot -= (double)(fmaxf(xd, 0.f) + __builtin_amdgcn_logf(1.f + exd));
  }
  const unsigned dpos = (unsigned)__popcll(__ballot(own && xd > 0.f));
  if (cb == 0 && h == 0) {   // s'_ii as the backward MFMA consumed it (bf16), 0 outside split 0
    const float sg = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(-xd) + 1.f);
    dsg[rg][r] = corr ? (float)(__bf16)sg : 0.f;
  }

  // ---- combine the four column blocks' partial dJ' (fixed order) through LDS, two
  // 32-column output blocks per pass; the diagonal term subtracted with the same
  // scaled z_i the backward products used, then the sqrt(log2 e) scale removed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may land in red
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);        // [cb-1][rg][2 * 16][64]
  float* dst = (sp == 0 ? a.dJd : a.dJd_extra + (long long)(sp - 1) * a.ngraphs * a.n * a.d) +
               (long long)g * a.n * a.d;
  const __bf16* zi = Jg + (long long)(rb * ROWS + 32 * rg) * DP;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (cb > 0) {
#pragma unroll
      for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          red[(((cb - 1) * 4 + rg) * 32 + qh * 16 + v) * 64 + lane] = acc[2 * pass + qh][v];
    }
    __syncthreads();
    if (cb == 0) {
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        const int c = 32 * (2 * pass + qh) + r;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          float o = acc[2 * pass + qh][v];
#pragma unroll
          for (int k = 0; k < 3; ++k) o += red[((k * 4 + rg) * 32 + qh * 16 + v) * 64 + lane];
          const int il = (v & 3) + 8 * (v >> 2) + 4 * h;   // D row within the row group
          const int i = i0 + il;
          if (i < a.n && c < a.d)
            dst[(long long)i * a.d + c] = (o - dsg[rg][il] * (float)zi[il * DP + c]) * kInvSqrtLog2e;
        }
      }
    }
    __syncthreads();
  }
  const double l = wave_sum_d(ltot);
  const unsigned wcnt = wave_sum_u(lcnt);
  if (lane == 0) { sl[w] = l; sc[w] = wcnt - dpos; }
  __syncthreads();
  if (tid == 0) {
    double tl = 0.0, tc = 0.0;
    for (int k = 0; k < NW; ++k) { tl += sl[k]; tc += (double)sc[k]; }
    if (corr) tl -= zzt_padded_pairs(a, rb);
    a.part[2 * blockIdx.x] = tl * (double)kLn2;
    a.part[2 * blockIdx.x + 1] = tc;
  }
}


// ---------------------------------------------------------------- bf16 MFMA, v9 (d = 64)
// v4's per-wave work (one 32 x 32 logit block per 128-column tile, the same signed
// epilogue) in HALF-size workgroups -- 512 threads = 2 row groups (64 rows i) x 4
// column blocks -- with v7's single dual-use LDS image per tile (16 KB at d = 64:
// ds_read_b128 rows for the forward, ds_read_b64_tr_b16 for the backward), so that
// TWO workgroups fit on a CU (~59 KB of LDS each, 4 waves per SIMD in all).  Each
// workgroup has its own barrier: the two drift apart, and one workgroup's epilogue
// VALU can issue under the other's MFMAs -- in v4 the 16 waves of the CU's one
// workgroup leave every tile barrier together, so the matrix and vector phases add up
// (DESIGN §5).  Tiles arrive by LDS-DMA into a 3-deep ring; the image holds
// z * sqrt(log2 e) (v7), so the backward result is divided by sqrt(log2 e) once.
// The tile loop: the workgroup's -z_i rows sit in an LDS image read again every tile;
// tile t + 1's DMA is issued in tile t, a full vmcnt(0) drain and a barrier end each tile.
constexpr int NTH9 = 512;
constexpr int ROWS9 = 64;
__device__ __forceinline__ int zoa64(int row, int ch) {   // [128][64] bf16 image, 16-byte chunk ch
  return 1024 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

// MEAS (variant >= 256, measurement build; results wrong): phase skips, variant >> 8 --
//   1 no epilogue, 4 no backward MFMAs, 2 the tile loop's skeleton (no epilogue and no
//   MFMA at all: the DMAs, waits, barriers and LDS operand reads stay), 8 no tile DMA
//   after each ring slot's first fill (the loop computes on stale tiles), 64 no tile at
//   all (the prologue, the row corrections, the combine and the stores remain), 16 the
//   symmetric-tile proxy: odd tiles only DMA
//   and barrier, even tiles run their epilogue once and the backward MFMAs twice (what a
//   J >= I tile kernel computes per logit block: forward 4 + epilogue + 2 x 4 backward
//   MFMAs over half the blocks; DESIGN §5 "symmetric tiles, measured")
typedef int zv4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void zkeep(const bf16x8& v) {   // MEAS: an operand read stays without its MFMA
  asm volatile("" ::"v"(__builtin_bit_cast(zv4i, v)));
}

template <bool MEAS>
__device__ __forceinline__ void zzt_v9_body(const ZztArgs& a) {
  constexpr int DP = 64, NT = NTH9, NW = NT / 64;
  const int skip = MEAS ? __builtin_amdgcn_readfirstlane(a.variant >> 8) : 0;
  constexpr int KS = DP / 16;          // forward k-steps
  constexpr int CB = DP / 32;          // backward 32-column output blocks
  constexpr int IMG = TJ2 * DP * 2;    // one [128][64] bf16 image, 16 KB
  constexpr int NS = 3;                // ring slots
  constexpr int BROWS = ROWS9 * DP * 2;   // the -z_i rows' LDS image
  __shared__ __attribute__((aligned(16))) char lds[NS * IMG + BROWS];   // ring, -z_i rows
  __shared__ float colsum[DP];
  __shared__ float csred[NT / DP][DP];
  __shared__ float dsg[2][32];
  __shared__ double sl[NW];
  __shared__ unsigned sc[NW];
  char* brows = lds + NS * IMG;
  const unsigned lds0 = (unsigned)(uintptr_t)(zlptr_t)lds;

  const int wgs = a.ngraphs * zrb(a) * 2;
  const int sp = blockIdx.x / wgs, bx = blockIdx.x - sp * wgs;
  const int nsplit = gridDim.x / wgs;
  const int g = bx % a.ngraphs, hb = bx / a.ngraphs;            // hb: 64-row block of the range
  const int rb = a.rb0 + (hb >> 1), half = hb & 1;              // its 128-row block and half
  const int r0 = rb * ROWS + ROWS9 * half;                      // first row
  const __bf16* Jg = reinterpret_cast<const __bf16*>(a.jrow) + (long long)g * a.npad * DP;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int rg = w & 1, cb = w >> 1;
  const int i0 = __builtin_amdgcn_readfirstlane(r0 + 32 * rg);
  const int i_me = i0 + r;
  const int ntot = a.npad / TJ2;
  const int t0 = sp * ntot / nsplit;
  const int t1 = (MEAS && (skip & 64)) ? t0 : (sp + 1) * ntot / nsplit;   // 64: no tile at all

  // tile t -> ring slot b: 16 pieces of 1 KB (8 rows each), wave w issues pieces w and w + 8
  int dsrc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int P = w + 8 * k;
    const int row = 8 * P + ((lane >> 2) & 7);
    const int ch = 4 * (lane >> 5) + ((lane & 3) ^ ((row >> 2) & 3));
    dsrc[k] = row * DP + 8 * ch;
  }
  auto dma = [&](int t, int b) {
    if (MEAS && (skip & 8) && t >= t0 + NS) return;   // every slot filled once, then no DMA
#pragma unroll
    for (int k = 0; k < 2; ++k)
      zdma16(Jg + (long long)t * TJ2 * DP + dsrc[k],
             __builtin_amdgcn_readfirstlane(lds0 + b * IMG + 1024 * (w + 8 * k)));
  };

  // ---- prologue: tile t0 in flight; -z_i rows; column sums
  dma(t0, 0);
  const int ja = 32 * cb + r, ia = 32 * rg + r;
  for (int idx = tid; idx < ROWS9 * (DP / 8); idx += NT) {
    const int row = idx >> 3, ch = idx & 7;
    const uint4 u = *reinterpret_cast<const uint4*>(Jg + (long long)(r0 + row) * DP + ch * 8);
    *reinterpret_cast<uint4*>(brows + zoa64(row, ch)) =
        make_uint4(u.x ^ 0x80008000u, u.y ^ 0x80008000u, u.z ^ 0x80008000u, u.w ^ 0x80008000u);
  }
  {
    const int nrb = a.npad / 64;
    const int k = tid % DP, grp = tid / DP;
    float s = 0.f;
    // eight partials in flight at a time, added in the same order (one load per loop trip
    // made every trip a dependent L2 round trip: 8 in a row at N = 4096)
    for (int p0 = grp; p0 < nrb; p0 += 8 * (NT / DP)) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)   // clamped, so the load is unconditional
        v[j] = a.colpart[((long long)g * nrb + min(p0 + j * (NT / DP), nrb - 1)) * DP + k];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (p0 + j * (NT / DP) < nrb) s += v[j];
    }
    csred[grp][k] = s;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid < DP) {
    float s = 0.f;
    for (int p = 0; p < NT / DP; ++p) s += csred[p][tid];
    colsum[tid] = s;
  }

  f32x16 acc[CB];
#pragma unroll
  for (int q = 0; q < CB; ++q)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[q][v] = 0.f;
  // forward operand bases (k-step s: base[s & 1] + 512 (s >> 1))
  const int fa0 = zoa64(ja, h), fa1 = zoa64(ja, 2 + h);
  const int fb0 = zoa64(ia, h), fb1 = zoa64(ia, 2 + h);
  auto brow = [&](int s) {   // the forward B operand of k-step s: -z_i chunk 2 s + h
    return *reinterpret_cast<const bf16x8*>(brows + ((s & 1) ? fb1 : fb0) + 512 * (s >> 1));
  };
  // backward transposed-read bases (v7's, 8-row groups of 1 KB): lane 4 qq + pp of group
  // gq supplies row 32 cb + 16 s + 8 t + 4 (gq >> 1) + qq, columns 32 q + 16 (gq & 1) + 4 pp
  const int gq = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
  const int c0 = 2 * (gq & 1) + (pp >> 1);
  const int tb0 = 1024 * (4 * cb) + 64 * (4 * (gq >> 1) + qq) + 16 * (c0 ^ (gq >> 1)) + 8 * (pp & 1);
  const int tb1 = 1024 * (4 * cb + 1) + 64 * (4 * (gq >> 1) + qq) + 16 * (c0 ^ ((gq >> 1) + 2)) + 8 * (pp & 1);
  auto fwd = [&](int b) {
    f32x16 X;
#pragma unroll
    for (int v = 0; v < 16; ++v) X[v] = 0.f;
    const char* T = lds + b * IMG;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(T + ((s & 1) ? fa1 : fa0) + 512 * (s >> 1));
      const bf16x8 bv = brow(s);
      if (MEAS && (skip & 2)) { zkeep(av); zkeep(bv); continue; }
      X = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, X, 0, 0, 0);
    }
    return X;
  };
  float lacc = 0.f;
  double ltot = 0.0;
  unsigned lcnt = 0;
  bool ovf = false;   // sticky per wave, as v4
  auto epi = [&](const f32x16& Y, bf16x8 (&sA)[2]) {   // v4's epilogue, y = -x
    if (MEAS && (skip & 3)) {
#pragma unroll
      for (int v = 0; v < 16; ++v) sA[v >> 3][v & 7] = (__bf16)Y[v];
      return;
    }
    float q[16], lt = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float e = __builtin_amdgcn_exp2f(Y[v]);
      q[v] = e + 1.f;
      sA[v >> 3][v & 7] = (__bf16)__builtin_amdgcn_rcpf(q[v]);
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const unsigned t01 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 1]),
                                                 __float_as_uint(Y[4 * g4]), 0x0C0C0703u);
      const unsigned t23 = __builtin_amdgcn_perm(__float_as_uint(Y[4 * g4 + 3]),
                                                 __float_as_uint(Y[4 * g4 + 2]), 0x07030C0Cu);
      lcnt += (unsigned)__builtin_popcount((t01 | t23) & 0x80808080u);
    }
    if (!ovf) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        lt += __builtin_amdgcn_logf((q[4 * p] * q[4 * p + 1]) * (q[4 * p + 2] * q[4 * p + 3]));
      ovf = __builtin_amdgcn_ballot_w64(!__builtin_isfinite(lt)) != 0;
    }
    if (__builtin_expect(ovf, 0)) {
      lt = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) lt += Y[v] > 24.f ? Y[v] : __builtin_amdgcn_logf(q[v]);
    }
    lacc += lt;
  };
  auto bwd = [&](int b, const bf16x8 (&sA)[2]) {
    if (MEAS && (skip & 4)) { lacc += (float)sA[0][0]; return; }
    const char* T = lds + b * IMG;
#pragma unroll
    for (int rep = 0; rep < ((MEAS && (skip & 16)) ? 2 : 1); ++rep)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < CB; ++q) {
        const bf16x8 bv = ztr_pair(T + tb0 + 2048 * s + 512 * q + 8 * rep, T + tb1 + 2048 * s + 512 * q + 8 * rep);
        if (MEAS && (skip & 2)) { zkeep(bv); continue; }
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sA[s], bv, acc[q], 0, 0, 0);
      }
  };
  // the tile loop.  Tile t in ring slot CUR: tile t + 1's DMA into the slot tile t - 2
  // left, forward, epilogue, backward; then the full drain (tile t + 1 landed) and the barrier.
  // (run stays a lambda, and this body a function of its own under the kernel: written
  // straight into the kernel the same code compiles to a different instruction order)
  auto run = [&]() {
    auto tile = [&](int t, auto cc) {
      constexpr int CUR = decltype(cc)::value;
      if (t + 1 < t1) dma(t + 1, (CUR + 1) % 3);
      const f32x16 Y = fwd(CUR);
      bf16x8 sA[2];
      epi(Y, sA);
      bwd(CUR, sA);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile t+1 landed
      __syncthreads();
    };
    for (int t = t0; t < t1; t += 3) {
      tile(t, std::integral_constant<int, 0>{});
      if (t + 1 < t1) tile(t + 1, std::integral_constant<int, 1>{});
      if (t + 2 < t1) tile(t + 2, std::integral_constant<int, 2>{});
      ltot += (double)lacc;   // keep the fp32 partial sums short
      lacc = 0.f;
    }
  };
  run();

  // ---- per-row corrections (row i_me; lanes r and r + 32 hold its two k halves)
  float xd = 0.f, xs = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const bf16x8 bv = brow(s);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float bb = (float)bv[e];
      xd += bb * bb;
      xs += bb * colsum[16 * s + 8 * h + e];
    }
  }
  xd += __shfl_xor(xd, 32, 64);
  xs += __shfl_xor(xs, 32, 64);
  xs = -xs;
  const bool row_valid = i_me < a.n;
  const bool corr = sp == 0;
  const bool own = cb == 0 && h == 0 && row_valid && corr;
  const float exd = __builtin_amdgcn_exp2f(-fabsf(xd));
  if (own) {
    ltot += (double)xs;
    ltot -= (double)(fmaxf(xd, 0.f) + __builtin_amdgcn_logf(1.f + exd));
  }
  const unsigned dpos = (unsigned)__popcll(__ballot(own && xd > 0.f));
  if (cb == 0 && h == 0) {   // s'_ii as the backward MFMA consumed it (bf16), 0 outside split 0
    const float sg = __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(-xd) + 1.f);
    dsg[rg][r] = corr ? (float)(__bf16)sg : 0.f;
  }

  // ---- combine the four column blocks' partial dJ (fixed order) through the ring's
  // first 48 KB; the diagonal term subtracted with the scaled z_i the backward products used,
  // then the sqrt(log2 e) scale removed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);        // [cb-1][rg][CB * 16][64]
  float* dst = (sp == 0 ? a.dJd : a.dJd_extra + (long long)(sp - 1) * a.ngraphs * a.n * a.d) +
               (long long)g * a.n * a.d;
  const __bf16* zi = Jg + (long long)(r0 + 32 * rg) * DP;
  // the diagonal term's z_i, all 32 loaded before the barrier (rows of the padded image,
  // in bounds for every lane): loaded inside the guarded store below, each element waited
  // for its own load and for the store before it, 32 memory round trips in a row
  float zd[CB][16];
  if (cb > 0) {
#pragma unroll
    for (int q = 0; q < CB; ++q)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        red[(((cb - 1) * 2 + rg) * (CB * 16) + q * 16 + v) * 64 + lane] = acc[q][v];
  } else {
#pragma unroll
    for (int q = 0; q < CB; ++q)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        zd[q][v] = (float)zi[((v & 3) + 8 * (v >> 2) + 4 * h) * DP + 32 * q + r];
  }
  __syncthreads();
  if (cb == 0) {
#pragma unroll
    for (int q = 0; q < CB; ++q) {
      const int c = 32 * q + r;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float o = acc[q][v];
#pragma unroll
        for (int k = 0; k < 3; ++k) o += red[((k * 2 + rg) * (CB * 16) + q * 16 + v) * 64 + lane];
        const int il = (v & 3) + 8 * (v >> 2) + 4 * h;   // D row within the row group
        const int i = i0 + il;
        if (i < a.n && c < a.d)
          dst[(long long)i * a.d + c] = (o - dsg[rg][il] * zd[q][v]) * kInvSqrtLog2e;
      }
    }
  }
  const double l = wave_sum_d(ltot);
  const unsigned wcnt = wave_sum_u(lcnt);
  if (lane == 0) { sl[w] = l; sc[w] = wcnt - dpos; }
  __syncthreads();
  if (tid == 0) {
    double tl = 0.0, tc = 0.0;
    for (int k = 0; k < NW; ++k) { tl += sl[k]; tc += (double)sc[k]; }
    if (corr) {   // padded pairs of this 64-row block: x = 0 exactly, softplus2(0) = 1 each
      const int valid = max(0, min(ROWS9, a.n - r0));
      tl -= (double)ROWS9 * a.npad - (double)valid * a.n;
    }
    a.part[2 * blockIdx.x] = tl * (double)kLn2;
    a.part[2 * blockIdx.x + 1] = tc;
  }
}

template <bool MEAS>
__global__ void __launch_bounds__(NTH9) __attribute__((amdgpu_waves_per_eu(4, 4)))
zzt_dense_bf16_v9(ZztArgs a) {
  zzt_v9_body<MEAS>(a);
}

// dJd += sum of the column-split partials (fixed order)
__global__ void zzt_split_sum_kernel(float* dJd, const float* extra, long long n, long long stride,
                                     int nextra) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v = dJd[i];
    for (int s = 0; s < nextra; ++s) v += extra[(long long)s * stride + i];
    dJd[i] = v;
  }
}

// dz = scale * (dz + ej)
__global__ void zzt_combine_kernel(float* dz, const float* ej, long long n, float norm) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) dz[i] = norm * (dz[i] + ej[i]);
}

// out = scale * (a + b)   (row-sharded combine: dJd rows of the range + edge terms)
__global__ void zzt_combine2_kernel(float* out, const float* a, const float* b, long long n, float scale) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = scale * (a[i] + b[i]);
}

// stats of a row range: rows * n pairs, the range's edges (rowptr[rows] - rowptr[0])
__global__ void zzt_stats_rows_kernel(const double* pd, int nd, const double* pe, int ne,
                                      const int* rowptr, int rows, int n, float norm,
                                      double* stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double dl = 0.0, dc = 0.0, el = 0.0, tp = 0.0;
  for (int k = 0; k < nd; ++k) { dl += pd[2 * k]; dc += pd[2 * k + 1]; }
  for (int k = 0; k < ne; ++k) { el += pe[2 * k]; tp += pe[2 * k + 1]; }
  const double nnz = (double)(rowptr[rows] - rowptr[0]);
  stats[0] = (double)norm * (dl + el + (double)rows * kSoftplusM1);
  stats[1] = (double)rows * n - nnz - dc + 2.0 * tp;
}

__global__ void zzt_stats_kernel(const double* pd, int nd, const double* pe, int ne,
                                 const int* rowptr, int ngraphs, int n, float norm,
                                 double* stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double dl = 0.0, dc = 0.0, el = 0.0, tp = 0.0;
  for (int k = 0; k < nd; ++k) { dl += pd[2 * k]; dc += pd[2 * k + 1]; }
  for (int k = 0; k < ne; ++k) { el += pe[2 * k]; tp += pe[2 * k + 1]; }
  const double nnz = (double)rowptr[(long long)ngraphs * n];
  const double pairs = (double)ngraphs * n * (double)n;
  stats[0] = (double)norm * (dl + el + (double)ngraphs * n * kSoftplusM1);
  stats[1] = pairs - nnz - dc + 2.0 * tp;
}

}  // namespace

int zzt_dp(int d) {
  if (d <= 32) return 32;
  if (d <= 64) return 64;
  if (d <= 128) return 128;
  return -1;
}
int zzt_npad(int n) { return (int)round_up(n, ROWS); }
int zzt_tsplit(int ngraphs, int n, int dtype) {
  return zzt_tsplit_blocks(ngraphs * (zzt_npad(n) / ROWS), n, dtype);
}
int zzt_tsplit_blocks(int wgs, int n, int dtype) {
  const int ntiles = zzt_npad(n) / TJ2, ncu = device_cu_count();
  if (dtype != SND_BF16 || wgs >= ncu) return 1;
  // up to 8 column splits: one C2 graph (32 row blocks) then fills 256 CUs (B = 1 step
  // 0.1546 -> 0.1512 ms against 4 splits; B = 2 unchanged at 4)
  return std::max(1, std::min({cdiv(ncu, wgs), 8, ntiles}));
}
// bf16 at dp = 64 is v9: two 64-row workgroups, and loss partials, per 128-row block
int zzt_wpb(int d, int dtype) { return (dtype == SND_BF16 && zzt_dp(d) == 64) ? 2 : 1; }
int zzt_dense_blocks(int ngraphs, int n, int d, int dtype) {
  return ngraphs * (zzt_npad(n) / ROWS) * zzt_tsplit(ngraphs, n, dtype) * zzt_wpb(d, dtype);
}

size_t zzt_staging_bytes(int ngraphs, int n, int d, int dtype) {
  const int dp = zzt_dp(d);
  const size_t es = dtype == SND_BF16 ? 2 : 4;
  const size_t img = round_up((size_t)ngraphs * zzt_npad(n) * dp * es, 256);
  return 2 * img + round_up((size_t)ngraphs * (zzt_npad(n) / 64) * dp * sizeof(float), 256);
}

ZztStage zzt_stage(void* base, int ngraphs, int n, int d, int dtype) {
  const int dp = zzt_dp(d);
  const size_t es = dtype == SND_BF16 ? 2 : 4;
  const size_t img = round_up((size_t)ngraphs * zzt_npad(n) * dp * es, 256);
  char* b = (char*)base;
  return ZztStage{b, b + img, (float*)(b + 2 * img)};
}

int launch_zzt_prep(const float* z, int ngraphs, int n, int d, int dtype, const ZztStage& st,
                    hipStream_t s) {
  void* jrow = st.jrow;
  void* jt = st.jt;
  const int dp = zzt_dp(d), npad = zzt_npad(n);
  dim3 grid(npad / 64, ngraphs);
#define SND_PREP(T, DPV)                                                                \
  hipLaunchKernelGGL((zzt_prep_kernel<T, DPV>), grid, dim3(256), 0, s, z, n, npad, d, \
                     (T*)jrow, (T*)jt, st.colpart)
  if (dtype == SND_BF16) {
    if (dp == 32) SND_PREP(__bf16, 32); else if (dp == 64) SND_PREP(__bf16, 64); else SND_PREP(__bf16, 128);
  } else {
    if (dp == 32) SND_PREP(float, 32); else if (dp == 64) SND_PREP(float, 64); else SND_PREP(float, 128);
  }
#undef SND_PREP
  SND_LAUNCH_CHECK("zzt_prep_kernel");
  return 0;
}

int launch_zzt_dense(const ZztArgs& a, int dtype, hipStream_t s, bool defer_split) {
  const int dp = zzt_dp(a.d);
  SND_CHECK_ARG(a.rb0 >= 0 && a.nrb >= 0 && a.rb0 + zrb(a) <= a.npad / ROWS,
                "zzt_dense: row blocks [%d, %d) outside the %d of the graph", a.rb0, a.rb0 + zrb(a),
                a.npad / ROWS);
  // 0 the (dtype, dp)'s kernel, 1 v1 (bf16), 256 * bits the default's measurement build
  const bool meas = a.variant >= 256 && (a.variant & 255) == 0;
  SND_CHECK_ARG(a.variant == 0 || a.variant == 1 || meas,
                "zzt_dense: unknown variant %d (0, 1 or 256 * measurement bits)", a.variant);
  const int ts = (dtype == SND_BF16 && a.variant == 0)
                     ? (a.tsplit > 0 ? a.tsplit : zzt_tsplit_blocks(a.ngraphs * zrb(a), a.n, dtype)) : 1;
  SND_CHECK_ARG(ts <= std::max(1, zzt_tsplit_blocks(a.ngraphs * zrb(a), a.n, dtype)),
                "zzt_dense: %d column splits > the %d the scratch is sized for", ts,
                zzt_tsplit_blocks(a.ngraphs * zrb(a), a.n, dtype));
  SND_CHECK_ARG(ts == 1 || a.dJd_extra, "zzt_dense: column splits need dJd_extra");
  SND_CHECK_ARG(a.nrb == 0 || a.ngraphs == 1, "zzt_dense: a row-block range needs one graph");
  dim3 grid(a.ngraphs * zrb(a) * ts);
  if (dtype != SND_BF16) {                            // f32 parity mode
    const size_t shm = 2 * 2 * (size_t)TJ * dp * sizeof(float);
    if (dp == 32) hipLaunchKernelGGL((zzt_dense_f32<32>), grid, dim3(NTH), shm, s, a);
    else if (dp == 64) hipLaunchKernelGGL((zzt_dense_f32<64>), grid, dim3(NTH), shm, s, a);
    else hipLaunchKernelGGL((zzt_dense_f32<128>), grid, dim3(NTH), shm, s, a);
  } else if (a.variant == 1) {                        // v1
    if (dp == 32) hipLaunchKernelGGL((zzt_dense_bf16<32>), grid, dim3(NTH), 0, s, a);
    else if (dp == 64) hipLaunchKernelGGL((zzt_dense_bf16<64>), grid, dim3(NTH), 0, s, a);
    else hipLaunchKernelGGL((zzt_dense_bf16<128>), grid, dim3(NTH), 0, s, a);
  } else if (dp == 32) {                              // v4; meas: phase skips / stamps, variant >> 8
    if (meas) hipLaunchKernelGGL((zzt_dense_bf16_v4<32, true>), grid, dim3(NTH2), 0, s, a);
    else hipLaunchKernelGGL((zzt_dense_bf16_v4<32, false>), grid, dim3(NTH2), 0, s, a);
  } else if (dp == 64) {                              // v9: two 64-row workgroups per row block
    const dim3 g9(grid.x * 2);
    if (meas) hipLaunchKernelGGL((zzt_dense_bf16_v9<true>), g9, dim3(NTH9), 0, s, a);
    else hipLaunchKernelGGL((zzt_dense_bf16_v9<false>), g9, dim3(NTH9), 0, s, a);
  } else {                                            // v7 (d = 128)
    if (meas) hipLaunchKernelGGL((zzt_dense_bf16_v7<true>), grid, dim3(NTH2), 0, s, a);
    else hipLaunchKernelGGL((zzt_dense_bf16_v7<false>), grid, dim3(NTH2), 0, s, a);
  }
  SND_LAUNCH_CHECK("zzt_dense");
  if (ts > 1 && !defer_split) {
    // the launch's rows only (a row-block range writes no other rows of the slabs)
    const long long r0 = (long long)a.rb0 * ROWS;
    const long long r1 = a.nrb ? std::min<long long>(a.n, r0 + (long long)a.nrb * ROWS) : a.n;
    const long long cnt = (long long)a.ngraphs * (r1 - r0) * a.d, total = (long long)a.ngraphs * a.n * a.d;
    hipLaunchKernelGGL(zzt_split_sum_kernel, dim3((unsigned)std::min<long long>(cdiv(cnt, 256), 4096)),
                       dim3(256), 0, s, a.dJd + r0 * a.d, a.dJd_extra + r0 * a.d, cnt, total, ts - 1);
    SND_LAUNCH_CHECK("zzt_split_sum_kernel");
  }
  return 0;
}

static int zzt_init_attributes_once() {
  // the f32 variants use up to 128 KiB of dynamic LDS
  hipError_t e = hipFuncSetAttribute((const void*)zzt_dense_f32<128>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
  if (e != hipSuccess) {
    set_error("zzt: hipFuncSetAttribute: %s", hipGetErrorString(e));
    return SND_ERR_HIP;
  }
  e = hipFuncSetAttribute((const void*)zzt_dense_f32<64>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
  if (e != hipSuccess) {
    set_error("zzt: hipFuncSetAttribute: %s", hipGetErrorString(e));
    return SND_ERR_HIP;
  }
  return 0;
}
// once per process, thread-safe (a function-local static's initialiser runs exactly once)
int zzt_init_attributes() {
  static const int rc = zzt_init_attributes_once();
  return rc;
}

}  // namespace snd

using namespace snd;

extern "C" size_t snd_zzt_ce_workspace(int n_graphs, int n, int d, int dtype) {
  if (zzt_dp(d) < 0 || n <= 0 || n_graphs <= 0) return 0;
  const long long rows = (long long)n_graphs * n;
  size_t b = round_up(zzt_staging_bytes(n_graphs, n, d, dtype), 256);
  b += round_up(rows * d * sizeof(float), 256);                               // ej
  b += round_up(2 * sizeof(double) * (size_t)zzt_dense_blocks(n_graphs, n, d, dtype), 256);
  b += round_up(2 * sizeof(double) * (size_t)edge_blocks((int)rows, d), 256);
  b += round_up((size_t)(zzt_tsplit(n_graphs, n, dtype) - 1) * rows * d * sizeof(float), 256);
  return b;
}

extern "C" int snd_zzt_ce(const float* z, int n_graphs, int n, int d, const int* rowptr,
                          const int* colidx, float pos_weight, float norm,
                          double* stats, float* dz, void* ws, size_t ws_bytes,
                          int dtype, snd_stream_t stream) {
  // colidx may be NULL for an edgeless batch (never dereferenced when nnz == 0)
  SND_CHECK_ARG(z && rowptr && stats && dz, "snd_zzt_ce: null operand");
  SND_CHECK_ARG(d == 16 || d == 32 || d == 64 || d == 128, "snd_zzt_ce: d=%d not in {16,32,64,128}", d);
  SND_CHECK_ARG(n > 0 && n_graphs > 0, "snd_zzt_ce: empty batch");
  SND_CHECK_ARG(dtype == SND_F32 || dtype == SND_BF16, "snd_zzt_ce: bad dtype");
  const size_t need = snd_zzt_ce_workspace(n_graphs, n, d, dtype);
  SND_CHECK_ARG(ws && ws_bytes >= need, "snd_zzt_ce: workspace %zu < %zu", ws_bytes, need);
  // edge_kernel reads z as float4, the dense kernels store float4 rows of dJd, the staging
  // images are read as 16-byte vectors
  SND_CHECK_ARG((((uintptr_t)z | (uintptr_t)dz | (uintptr_t)ws) & 15) == 0,
                "snd_zzt_ce: z, dz and the workspace must be 16-byte aligned");
  SND_TRY(zzt_init_attributes());
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)ws;
  const ZztStage stg = zzt_stage(p, n_graphs, n, d, dtype);
  p += round_up(zzt_staging_bytes(n_graphs, n, d, dtype), 256);
  const long long rows = (long long)n_graphs * n;
  float* ej = (float*)p;
  p += round_up(rows * d * sizeof(float), 256);
  double* pd = (double*)p;
  p += round_up(2 * sizeof(double) * (size_t)zzt_dense_blocks(n_graphs, n, d, dtype), 256);
  double* pe = (double*)p;
  p += round_up(2 * sizeof(double) * (size_t)edge_blocks((int)rows, d), 256);
  float* extra = (float*)p;

  SND_TRY(launch_zzt_prep(z, n_graphs, n, d, dtype, stg, s));
  ZztArgs a{stg.jrow, stg.jt, n, zzt_npad(n), n_graphs, d, dz, pd, stg.colpart, 0, extra};
  SND_TRY(launch_zzt_dense(a, dtype, s));
  EdgeArgs e{rowptr, colidx, (int)rows, z, d, pos_weight, ej, pe};
  SND_TRY(launch_edge(e, s));
  // d(sum CE)/dz_i = sum_j (G_ij + G_ji) z_j = 2 norm (dJd_i + ej_i)
  hipLaunchKernelGGL(zzt_combine_kernel, dim3(1024), dim3(256), 0, s, dz, ej, rows * d, 2.f * norm);
  SND_LAUNCH_CHECK("zzt_combine_kernel");
  hipLaunchKernelGGL(zzt_stats_kernel, dim3(1), dim3(64), 0, s, pd,
                     zzt_dense_blocks(n_graphs, n, d, dtype), pe, edge_blocks((int)rows, d), rowptr,
                     n_graphs, n, norm, stats);
  SND_LAUNCH_CHECK("zzt_stats_kernel");
  return 0;
}

// ---------------------------------------------------------------- row-sharded CE
// One graph's rows [row0, row1) against all of its columns: every rank of a
// row-sharded zz^T owns a contiguous row range, and because L is symmetric its
// dz rows need no reduction across ranks (d CE / dz_i = 2 norm sum_j G_ij z_j).
static void zrows_layout(int n, int d, int row0, int row1, int dtype, size_t* off, size_t* total) {
  const int rows = row1 - row0;
  const int rb0 = row0 / 128, nrb = (int)cdiv(row1, 128) - rb0;
  const int ts = zzt_tsplit_blocks(nrb, n, dtype);
  size_t b = 0;
  off[0] = b; b += round_up(zzt_staging_bytes(1, n, d, dtype), 256);              // images
  off[1] = b; b += round_up((size_t)n * d * sizeof(float), 256);                  // dJd (full rows)
  off[2] = b; b += round_up((size_t)rows * d * sizeof(float), 256);               // ej
  off[3] = b; b += round_up(2 * sizeof(double) * (size_t)nrb * ts * zzt_wpb(d, dtype), 256);   // dense partials
  off[4] = b; b += round_up(2 * sizeof(double) * (size_t)edge_blocks(rows, d), 256);
  off[5] = b; b += round_up((size_t)std::max(0, ts - 1) * n * d * sizeof(float), 256);   // splits
  *total = b;
}

extern "C" size_t snd_zzt_ce_rows_workspace(int n, int d, int row0, int row1, int dtype) {
  if (zzt_dp(d) < 0 || n <= 0 || row0 < 0 || row1 <= row0 || row1 > n) return 0;
  size_t off[6], total;
  zrows_layout(n, d, row0, row1, dtype, off, &total);
  return total;
}

extern "C" int snd_zzt_ce_rows(const float* z, int n, int d, int row0, int row1,
                               const int* rowptr, const int* colidx, float pos_weight, float norm,
                               double* stats, float* dz, void* ws, size_t ws_bytes, int dtype,
                               snd_stream_t stream) {
  SND_CHECK_ARG(z && rowptr && stats && dz, "snd_zzt_ce_rows: null operand");
  SND_CHECK_ARG(d == 16 || d == 32 || d == 64 || d == 128, "snd_zzt_ce_rows: d=%d not in {16,32,64,128}", d);
  SND_CHECK_ARG(n > 0 && 0 <= row0 && row0 < row1 && row1 <= n,
                "snd_zzt_ce_rows: rows [%d, %d) outside [0, %d)", row0, row1, n);
  SND_CHECK_ARG(row0 % 128 == 0 && (row1 % 128 == 0 || row1 == n),
                "snd_zzt_ce_rows: row range [%d, %d) not on 128-row blocks", row0, row1);
  SND_CHECK_ARG(dtype == SND_F32 || dtype == SND_BF16, "snd_zzt_ce_rows: bad dtype");
  size_t off[6], need;
  zrows_layout(n, d, row0, row1, dtype, off, &need);
  SND_CHECK_ARG(ws && ws_bytes >= need, "snd_zzt_ce_rows: workspace %zu < %zu", ws_bytes, need);
  // edge_kernel reads z as float4, the dense kernels store float4 rows of dJd, the staging
  // images are read as 16-byte vectors
  SND_CHECK_ARG((((uintptr_t)z | (uintptr_t)dz | (uintptr_t)ws) & 15) == 0,
                "snd_zzt_ce_rows: z, dz and the workspace must be 16-byte aligned");
  SND_TRY(zzt_init_attributes());
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)ws;
  const int rows = row1 - row0;
  const int rb0 = row0 / 128, nrb = (int)cdiv(row1, 128) - rb0;
  const ZztStage stg = zzt_stage(p + off[0], 1, n, d, dtype);
  float* djd = (float*)(p + off[1]);
  float* ej = (float*)(p + off[2]);
  double* pd = (double*)(p + off[3]);
  double* pe = (double*)(p + off[4]);
  SND_TRY(launch_zzt_prep(z, 1, n, d, dtype, stg, s));
  ZztArgs a{stg.jrow, stg.jt, n, zzt_npad(n), 1, d, djd, pd, stg.colpart, 0, (float*)(p + off[5])};
  a.rb0 = rb0;
  a.nrb = nrb;
  SND_TRY(launch_zzt_dense(a, dtype, s));
  EdgeArgs e{rowptr, colidx, rows, z, d, pos_weight, ej, pe};
  e.row0 = row0;
  SND_TRY(launch_edge(e, s));
  hipLaunchKernelGGL(zzt_combine2_kernel, dim3(1024), dim3(256), 0, s, dz, djd + (long long)row0 * d, ej,
                     (long long)rows * d, 2.f * norm);
  SND_LAUNCH_CHECK("zzt_combine2_kernel");
  const int ts = zzt_tsplit_blocks(nrb, n, dtype == SND_BF16 ? SND_BF16 : dtype);
  hipLaunchKernelGGL(zzt_stats_rows_kernel, dim3(1), dim3(64), 0, s, pd,
                     nrb * ((dtype == SND_BF16) ? ts : 1) * zzt_wpb(d, dtype), pe, edge_blocks(rows, d), rowptr, rows, n,
                     norm, stats);
  SND_LAUNCH_CHECK("zzt_stats_rows_kernel");
  return 0;
}
