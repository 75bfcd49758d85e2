// Chebyshev moments of the spectral density of the normalised Laplacian (snd_graph_spectrum):
// per graph block b of a block-diagonal CSR, mu_k = tr T_k(M_b), M = L - I = -D^{-1/2} A D^{-1/2}
// on the mutual-edge graph (an isolated node keeps eigenvalue 0 of L: (M x)_i = -x_i), either
// exactly (the n unit vectors as probes) or as a Hutchinson estimate over Rademacher probes.
// Everything is fp64; the only atomics are the integer counts of the prep kernel.
//
// gs_prep_kernel: a wave per row i.  Each in-block entry j != i is looked up in row j by the
// whole wave (snd_gmotifs.hip's test): found -> a mutual entry, flag 1.0 in wgt[e], else a
// one-way arc, flag 0.0 (as for out-of-block entries and self loops).  deg[i] = the mutual
// entries; sum of degrees, isolated nodes and one-way arcs go to 64-bit integer accumulators.
// gs_weight_kernel: a wave per row; a flagged entry becomes 1 / sqrt(d_i d_j).  The wave of a
// graph's first row writes info[b].
//
// Probes run in column blocks of kGsWidth = 32: the state is [rows, 32] doubles, a row is 256 B.
// With t_0 = V (the block's probe columns), t_1 = M t_0, t_{s+1} = 2 M t_s - t_{s-1}, step s
// forms t_{s+1} over t_{s-1} in place (it reads only its own element of that buffer) and the dots
//   b_s = <t_{s+1}, t_s>,  a_{s+1} = <t_{s+1}, t_{s+1}>,
// which give mu_{2s+1} = 2 b_s - mu_1 (mu_1 = b_0) and mu_{2s+2} = 2 a_{s+1} - mu_0 because M is
// symmetric: K moments take K / 2 applications of M.
//
// Global path: gs_init_kernel writes t_0; per step gs_step_kernel (a 256-thread workgroup owns
// 8 rows x 32 columns; SpMM row, axpy and both dots fused; its two partial dots go to its slot
// of a slab) and gs_reduce_kernel (a wave per graph sums the graph's slots in a fixed order and
// adds them to the raw moments: launches of one stream, so the blocks add in stream order).
// LDS path (n <= 64): gs_lds_kernel, one launch per probe block, a workgroup per graph holds
// both state buffers, the graph's weights and local columns in LDS and runs every step with one
// barrier each; a graph whose CSR entries exceed the staged capacity reads them from global
// memory instead (same launch, same arithmetic order).  gs_final_kernel turns the raw dot sums
// into moments in place.
#include "snd_gspectrum.hpp"

namespace snd {

__device__ __forceinline__ double gs_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int gs_row_end(const GraphSpectrumArgs& a, int end) {
  return (long long)end < a.nnz_cap ? end : (int)a.nnz_cap;
}

// Entry (node i, probe r) of graph g's probe matrix.
__device__ __forceinline__ double gs_probe(const GraphSpectrumArgs& a, int g, int i, int r) {
  if (a.n_probes == 0) return r == i ? 1.0 : 0.0;
  if (r >= a.n_probes) return 0.0;
  const uint4 x = philox4x32_10(make_uint4((unsigned)i, (unsigned)r, (unsigned)g, kGsPhiloxTag),
                                make_uint2((unsigned)a.seed, (unsigned)(a.seed >> 32)));
  return (x.x & 1u) ? -1.0 : 1.0;
}

__global__ void __launch_bounds__(256) gs_prep_kernel(GraphSpectrumArgs a) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)a.n * a.ngraphs;
  const unsigned n = (unsigned)a.n;
  for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (long long)gridDim.x * 4) {
    const long long g = i / a.n;
    const unsigned cbase = (unsigned)(g * a.n), li = (unsigned)(i - g * a.n);
    const int* rp = a.rowptr + (long long)cbase;
    const int beg = a.rowptr[i], end = gs_row_end(a, a.rowptr[i + 1]);
    unsigned cnt = 0, one = 0;
    for (int e0 = beg; e0 < end; e0 += 64) {
      const int e = e0 + lane;
      unsigned lc = ~0u;
      if (e < end) lc = (unsigned)a.colidx[e] - cbase;
      const bool cand = lc < n && lc != li;
      bool mut = false;
      unsigned long long todo = __ballot(cand);
      while (todo) {                             // row j of each candidate: is i in it?
        const int k = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const unsigned j = (unsigned)__builtin_amdgcn_readlane((int)lc, k);
        const int jb = rp[j], je = gs_row_end(a, rp[j + 1]);
        bool f = false;
        for (int ee = jb + lane; ee < je; ee += 64) f |= (unsigned)a.colidx[ee] == (unsigned)i;
        const bool found = __ballot(f) != 0ull;
        if (lane == k) mut = found;
      }
      if (e < end) a.wgt[e] = (cand && mut) ? 1.0 : 0.0;
      cnt += (unsigned)__popcll(__ballot(cand && mut));
      one += (unsigned)__popcll(__ballot(cand && !mut));
    }
    if (lane == 0) {
      a.deg[i] = (int)cnt;
      unsigned long long* acc = a.acc + g * 4;
      if (cnt) atomicAdd(&acc[0], (unsigned long long)cnt);
      else atomicAdd(&acc[1], 1ull);
      if (one) atomicAdd(&acc[2], (unsigned long long)one);
    }
  }
}

__global__ void __launch_bounds__(256) gs_weight_kernel(GraphSpectrumArgs a) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)a.n * a.ngraphs;
  const unsigned n = (unsigned)a.n;
  for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (long long)gridDim.x * 4) {
    const long long g = i / a.n;
    const unsigned cbase = (unsigned)(g * a.n);
    const int beg = a.rowptr[i], end = gs_row_end(a, a.rowptr[i + 1]);
    const double di = (double)a.deg[i];
    for (int e = beg + lane; e < end; e += 64) {
      if (a.wgt[e] != 0.0) {
        const unsigned lc = (unsigned)a.colidx[e] - cbase;        // in block: the flag says so
        const double dj = (double)a.deg[(long long)cbase + (lc < n ? lc : 0u)];
        a.wgt[e] = 1.0 / sqrt(di * dj);
      }
    }
    if (i == g * a.n && lane == 0) {
      const unsigned long long* acc = a.acc + g * 4;
      long long* out = a.info + g * 4;
      out[0] = (long long)(acc[0] / 2);
      out[1] = (long long)acc[1];
      out[2] = (long long)acc[2];
      out[3] = a.n_probes > 0 ? a.n_probes : a.n;
    }
  }
}

__global__ void __launch_bounds__(256) gs_init_kernel(GraphSpectrumArgs a, int pblock, double* __restrict__ t0) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = idx >> 5;
  if (row >= (long long)a.n * a.ngraphs) return;
  const int g = (int)(row / a.n), li = (int)(row - (long long)g * a.n);
  t0[idx] = gs_probe(a, g, li, pblock * kGsWidth + (int)(idx & 31));
}

// One recurrence step on the global state: nxt = (first ? 1 : 2) M cur - (first ? 0 : nxt).
__global__ void __launch_bounds__(256) gs_step_kernel(GraphSpectrumArgs a, const double* __restrict__ cur,
                                                      double* __restrict__ nxt, int first) {
  __shared__ double sPart[2][4];
  const int tid = threadIdx.x, c = tid & 31;
  const int g = blockIdx.x / a.tiles, tile = blockIdx.x - g * a.tiles;
  const int r = tile * kGsTileRows + (tid >> 5);
  const unsigned n = (unsigned)a.n;
  const long long cbase = (long long)g * a.n;
  double pa = 0.0, pb = 0.0;
  if (r < a.n) {
    const long long row = cbase + r;
    const double own = cur[row * kGsWidth + c];
    double acc = own;                                            // an isolated node: M x = -x
    if (a.deg[row] > 0) {
      acc = 0.0;
      const int beg = a.rowptr[row], end = gs_row_end(a, a.rowptr[row + 1]);
      for (int e = beg; e < end; ++e) {
        const unsigned lc = (unsigned)a.colidx[e] - (unsigned)cbase;
        acc += a.wgt[e] * cur[(cbase + (lc < n ? lc : 0u)) * kGsWidth + c];   // weight 0 unless in block
      }
    }
    const double tn = first ? -acc : -2.0 * acc - nxt[row * kGsWidth + c];
    nxt[row * kGsWidth + c] = tn;
    pb = tn * own;
    pa = tn * tn;
  }
  pb = gs_wave_sum(pb);
  pa = gs_wave_sum(pa);
  if ((tid & 63) == 0) {
    sPart[0][tid >> 6] = pb;
    sPart[1][tid >> 6] = pa;
  }
  __syncthreads();
  if (tid < 2) a.slab[(long long)blockIdx.x * 2 + tid] = ((sPart[tid][0] + sPart[tid][1]) + sPart[tid][2]) + sPart[tid][3];
}

__global__ void __launch_bounds__(64) gs_reduce_kernel(GraphSpectrumArgs a, int step) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const double* sl = a.slab + (long long)g * a.tiles * 2;
  double sb = 0.0, sa = 0.0;
  for (int t = lane; t < a.tiles; t += 64) {
    sb += sl[2 * t];
    sa += sl[2 * t + 1];
  }
  sb = gs_wave_sum(sb);
  sa = gs_wave_sum(sa);
  if (lane == 0) {
    double* m = a.moments + (long long)g * a.n_moments;
    m[2 * step + 1] += sb;
    if (2 * step + 2 < a.n_moments) m[2 * step + 2] += sa;
  }
}

// The whole recurrence of one probe block of one graph in LDS.
__global__ void __launch_bounds__(256) gs_lds_kernel(GraphSpectrumArgs a, int pblock) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sRaw[];
  const int tid = threadIdx.x, c = tid & 31, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, n = a.n, K = a.n_moments;
  const int elems = n * kGsWidth;
  double* sA = reinterpret_cast<double*>(sRaw);
  double* sB = sA + elems;
  double* sMom = sB + elems;                     // [K] raw dot sums of this block
  double* sPart = sMom + K;                      // [2 sets][2 dots][4 waves]
  double* sW = sPart + 16;                       // [lds_cap]
  int* sRp = reinterpret_cast<int*>(sW + a.lds_cap);              // [n + 1] offsets into sW / sC
  unsigned short* sC = reinterpret_cast<unsigned short*>(sRp + ((n + 2) / 2) * 2);   // [lds_cap]

  const long long cbase = (long long)g * n;
  const int* rp = a.rowptr + cbase;
  const int gbeg = rp[0], gend = gs_row_end(a, rp[n]);
  const int cnt = gend - gbeg;
  const bool staged = cnt >= 0 && cnt <= a.lds_cap;              // workgroup-uniform
  if (staged) {
    for (int e = tid; e < cnt; e += 256) {
      const unsigned lc = (unsigned)a.colidx[gbeg + e] - (unsigned)cbase;
      sW[e] = a.wgt[gbeg + e];
      sC[e] = (unsigned short)(lc < (unsigned)n ? lc : 0u);
    }
    for (int r = tid; r <= n; r += 256) {
      const int o = gs_row_end(a, rp[r]) - gbeg;
      sRp[r] = o < 0 ? 0 : (o > cnt ? cnt : o);
    }
  }
  for (int idx = tid; idx < elems; idx += 256) sA[idx] = gs_probe(a, g, idx >> 5, pblock * kGsWidth + c);
  for (int k = tid; k < K; k += 256) sMom[k] = 0.0;
  __syncthreads();

  const int steps = K / 2;
  for (int s = 0; s < steps; ++s) {
    const double* cur = (s & 1) ? sB : sA;
    double* nxt = (s & 1) ? sA : sB;
    double pa = 0.0, pb = 0.0;
    for (int idx = tid; idx < elems; idx += 256) {
      const int r = idx >> 5;
      const double own = cur[idx];
      double acc = own;
      if (a.deg[cbase + r] > 0) {
        acc = 0.0;
        if (staged) {
          const int beg = sRp[r], end = sRp[r + 1];
          for (int e = beg; e < end; ++e) acc += sW[e] * cur[(int)sC[e] * kGsWidth + c];
        } else {
          const int beg = rp[r], end = gs_row_end(a, rp[r + 1]);
          for (int e = beg; e < end; ++e) {
            const unsigned lc = (unsigned)a.colidx[e] - (unsigned)cbase;
            acc += a.wgt[e] * cur[(int)(lc < (unsigned)n ? lc : 0u) * kGsWidth + c];
          }
        }
      }
      const double tn = s == 0 ? -acc : -2.0 * acc - nxt[idx];
      nxt[idx] = tn;
      pb += tn * own;
      pa += tn * tn;
    }
    pb = gs_wave_sum(pb);
    pa = gs_wave_sum(pa);
    double* part = sPart + (s & 1) * 8;
    if (lane == 0) {
      part[wave] = pb;
      part[4 + wave] = pa;
    }
    __syncthreads();
    if (tid == 0) {
      sMom[2 * s + 1] = ((part[0] + part[1]) + part[2]) + part[3];
      if (2 * s + 2 < K) sMom[2 * s + 2] = ((part[4] + part[5]) + part[6]) + part[7];
    }
  }
  __syncthreads();
  double* m = a.moments + (long long)g * K;
  for (int k = tid; k < K; k += 256) m[k] += sMom[k];            // one workgroup per graph and launch
}

// Raw dot sums -> moments, in place: mu_0 = n, mu_1 = b_0, mu_{2s+1} = 2 b_s - mu_1,
// mu_{2s+2} = 2 a_{s+1} - mu_0; a probe estimate is the mean over the probes.
__global__ void __launch_bounds__(64) gs_final_kernel(GraphSpectrumArgs a) {
  const int g = blockIdx.x, lane = threadIdx.x;
  double* m = a.moments + (long long)g * a.n_moments;
  const double scale = a.n_probes > 0 ? (double)a.n_probes : 1.0;
  const double mu0 = (double)a.n, mu1 = m[1] / scale;            // every lane reads m[1] before lane 1 stores it
  for (int k = lane; k < a.n_moments; k += 64) {
    const double v = m[k] / scale;
    m[k] = k == 0 ? mu0 : k == 1 ? mu1 : (k & 1) ? 2.0 * v - mu1 : 2.0 * v - mu0;
  }
}

int launch_graph_spectrum(const GraphSpectrumArgs& a, bool use_lds, hipStream_t s) {
  const long long rows = (long long)a.n * a.ngraphs;
  const long long step_blocks = (long long)a.tiles * a.ngraphs;
  SND_CHECK_ARG(step_blocks < (1LL << 31), "snd_graph_spectrum: %lld workgroups", step_blocks);
  if (hipMemsetAsync(a.acc, 0, (size_t)a.ngraphs * 4 * 8, s) != hipSuccess ||
      hipMemsetAsync(a.moments, 0, (size_t)a.ngraphs * a.n_moments * 8, s) != hipSuccess) {
    set_error("snd_graph_spectrum: memset failed");
    return SND_ERR_HIP;
  }
  const long long want = (rows + 3) / 4, most = 64LL * device_cu_count();
  const dim3 prep((unsigned)(want < most ? want : most));
  hipLaunchKernelGGL(gs_prep_kernel, prep, dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("gs_prep_kernel");
  hipLaunchKernelGGL(gs_weight_kernel, prep, dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("gs_weight_kernel");

  const int blocks = graph_spectrum_blocks(a.n, a.n_probes), steps = graph_spectrum_steps(a.n_moments);
  if (use_lds) {
    const size_t lds = graph_spectrum_lds_bytes(a.n, a.n_moments);
    for (int p = 0; p < blocks; ++p) {
      hipLaunchKernelGGL(gs_lds_kernel, dim3((unsigned)a.ngraphs), dim3(256), lds, s, a, p);
      SND_LAUNCH_CHECK("gs_lds_kernel");
    }
  } else {
    double* buf[2] = {a.state, a.state + rows * kGsWidth};
    const dim3 init((unsigned)((rows * kGsWidth + 255) / 256));
    for (int p = 0; p < blocks; ++p) {
      hipLaunchKernelGGL(gs_init_kernel, init, dim3(256), 0, s, a, p, buf[0]);
      SND_LAUNCH_CHECK("gs_init_kernel");
      for (int k = 0; k < steps; ++k) {
        hipLaunchKernelGGL(gs_step_kernel, dim3((unsigned)step_blocks), dim3(256), 0, s, a, buf[k & 1],
                           buf[(k + 1) & 1], k == 0 ? 1 : 0);
        SND_LAUNCH_CHECK("gs_step_kernel");
        hipLaunchKernelGGL(gs_reduce_kernel, dim3((unsigned)a.ngraphs), dim3(64), 0, s, a, k);
        SND_LAUNCH_CHECK("gs_reduce_kernel");
      }
    }
  }
  hipLaunchKernelGGL(gs_final_kernel, dim3((unsigned)a.ngraphs), dim3(64), 0, s, a);
  SND_LAUNCH_CHECK("gs_final_kernel");
  return 0;
}

static size_t gs_acc_bytes(int n_graphs) { return (size_t)round_up((long long)n_graphs * 4 * 8, 16); }
static size_t gs_wgt_bytes(long long nnz_cap) { return (size_t)round_up((nnz_cap > 0 ? nnz_cap : 1) * 8, 16); }
static size_t gs_state_bytes(int n_graphs, int n) { return (size_t)n_graphs * n * kGsWidth * 8 * 2; }
static size_t gs_slab_bytes(int n_graphs, int n) {
  return (size_t)round_up((long long)n_graphs * graph_spectrum_tiles(n) * 2 * 8, 16);
}
static size_t gs_deg_bytes(int n_graphs, int n) { return (size_t)round_up((long long)n_graphs * n * 4, 16); }

}  // namespace snd

extern "C" size_t snd_graph_spectrum_workspace(int n_graphs, int n, long long nnz_cap) {
  using namespace snd;
  if (n_graphs < 1 || n < 1 || n > kGsMaxN || (long long)n * n_graphs >= (1LL << 31) || nnz_cap < 0) return 0;
  return gs_acc_bytes(n_graphs) + gs_wgt_bytes(nnz_cap) + gs_state_bytes(n_graphs, n) + gs_slab_bytes(n_graphs, n) +
         gs_deg_bytes(n_graphs, n);
}

extern "C" int snd_graph_spectrum(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                                  int n_moments, int n_probes, unsigned long long seed, int flags, double* moments,
                                  long long* info, void* workspace, size_t workspace_bytes, snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(n_graphs >= 1, "snd_graph_spectrum: n_graphs=%d < 1", n_graphs);
  SND_CHECK_ARG(n >= 1 && n <= kGsMaxN, "snd_graph_spectrum: n=%d not in [1, %d]", n, kGsMaxN);
  SND_CHECK_ARG((long long)n * n_graphs < (1LL << 31), "snd_graph_spectrum: n=%d x %d graphs too large", n, n_graphs);
  SND_CHECK_ARG(nnz_cap >= 0, "snd_graph_spectrum: nnz_cap=%lld < 0", nnz_cap);
  SND_CHECK_ARG(n_moments >= 2 && n_moments <= kGsMaxMoments, "snd_graph_spectrum: n_moments=%d not in [2, %d]",
                n_moments, kGsMaxMoments);
  SND_CHECK_ARG(n_probes >= 0, "snd_graph_spectrum: n_probes=%d < 0", n_probes);
  SND_CHECK_ARG((flags & ~SND_SPECTRUM_FORCE_GLOBAL) == 0, "snd_graph_spectrum: unknown flags 0x%x", flags);
  SND_CHECK_ARG(rowptr && moments && info, "snd_graph_spectrum: null operand");
  SND_CHECK_ARG(colidx || nnz_cap == 0, "snd_graph_spectrum: colidx is NULL with nnz_cap=%lld", nnz_cap);
  const size_t need = snd_graph_spectrum_workspace(n_graphs, n, nnz_cap);
  SND_CHECK_ARG(workspace && workspace_bytes >= need, "snd_graph_spectrum: workspace %zu < %zu", workspace_bytes,
                need);
  SND_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "snd_graph_spectrum: workspace not 8-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  GraphSpectrumArgs a{};
  a.rowptr = rowptr;
  a.colidx = colidx;
  a.nnz_cap = nnz_cap;
  a.n = n;
  a.ngraphs = n_graphs;
  a.n_moments = n_moments;
  a.n_probes = n_probes;
  a.seed = seed;
  a.moments = moments;
  a.info = info;
  a.acc = reinterpret_cast<unsigned long long*>(ws);
  ws += gs_acc_bytes(n_graphs);
  a.wgt = reinterpret_cast<double*>(ws);
  ws += gs_wgt_bytes(nnz_cap);
  a.state = reinterpret_cast<double*>(ws);
  ws += gs_state_bytes(n_graphs, n);
  a.slab = reinterpret_cast<double*>(ws);
  ws += gs_slab_bytes(n_graphs, n);
  a.deg = reinterpret_cast<int*>(ws);
  a.tiles = graph_spectrum_tiles(n);
  a.lds_cap = graph_spectrum_lds_cap(n, n_moments);
  const bool use_lds = n <= kGsLdsMaxN && !(flags & SND_SPECTRUM_FORCE_GLOBAL);
  return launch_graph_spectrum(a, use_lds, (hipStream_t)stream);
}
