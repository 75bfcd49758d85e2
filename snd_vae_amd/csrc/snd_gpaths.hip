// Path statistics of a block-diagonal CSR (snd_graph_paths): weak components, BFS hop
// distances and fp32 shortest routes of B graphs x n nodes, from the CSR that DeviceBatch
// holds or snd_zzt_edges writes, and the node coordinates.  Three kernels on one stream:
//
// gp_edge_len_kernel (with coords): one fp32 length per CSR entry into the workspace, a wave
// per row, coalesced with colidx.  Every later use reads that value, so a route is a sum of
// the same numbers whichever lane relaxes the arc.
//
// gp_components_kernel: a workgroup per graph (a thread per node, up to 1024), labels in
// LDS.  label[i] starts at i and only ever falls to the id of a node of i's weak component.  A sweep hooks along every arc, both
// ways and on the labels' own labels (atomicMin), then every node follows its label chain to
// its end; sweeps repeat until one changes nothing.  Then label is constant on a component
// and equals its smallest member.  Sizes are counted per label in LDS.
//
// gp_paths_kernel: a wave per source; its hop array and BFS queue (16-bit) and its route
// array (fp32 bit patterns) live in LDS.  BFS: the wave takes up to 64 queued nodes at a
// time, a lane each reads their row bounds, then the lanes stride together over each row's
// colidx.  An unseen column is claimed by writing the lane id into its hop slot (marks are
// >= 0x8000, hop counts < 0x8000): of the lanes holding one column (duplicate entries) the
// one whose mark stays appends it, at a ballot / popcount prefix.  Routes: sweeps over the
// queue (the reachable nodes in BFS order) relax every arc with an LDS atomicMin on the
// float's bit pattern (d >= 0: unsigned order is float order) until a sweep lowers nothing.
// fl(d + w) is monotone, so the fixed point is unique: the result does not depend on which
// lane wins.  Epilogue: hop and detour bins into the workgroup's LDS histograms, flushed with
// 64-bit vector atomics, as graph_stats_kernel flushes.
//
// Work: sources x arcs column ids for the BFS, and that per relaxation sweep.
#include "snd_gpaths.hpp"

#include <cmath>
#include <mutex>

namespace snd {

constexpr unsigned kGpInf = 0x7F800000u;       // +inf
constexpr unsigned kGpUnseen = 0xFFFFu;
constexpr unsigned kGpMark = 0x8000u;

// ||a - b||_2 over sd <= 3 coordinates, every rounding spelled out: the edge lengths and the
// straight-line distances of the detour are formed alike.
__device__ __forceinline__ float gp_dist(const float* a, const float* b, int sd) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < sd) {
      const float d = __fsub_rn(a[k], b[k]);
      s = __fadd_rn(s, __fmul_rn(d, d));
    }
  }
  return __fsqrt_rn(s);
}

// min(max(floor((route / e - 1) scale), 0), 255); clamped in float and on the integer, so
// no coordinate can address outside the histogram (a NaN goes to bin 0).
__device__ __forceinline__ unsigned gp_detour_bin(float route, float e, float scale) {
  const float v = __fmul_rn(__fsub_rn(__fdiv_rn(route, e), 1.f), scale);
  const float t = fminf(fmaxf(floorf(v), 0.f), (float)(kGpBins - 1));
  return min((unsigned)t, (unsigned)kGpBins - 1u);
}

__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

__device__ __forceinline__ void gp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(256) gp_edge_len_kernel(GraphPathsArgs a) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)a.n * a.ngraphs;
  const unsigned n = (unsigned)a.n;
  for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (long long)gridDim.x * 4) {
    const unsigned cbase = (unsigned)(i / a.n * a.n);
    const int beg = a.rowptr[i], end = a.rowptr[i + 1];
    const float* ci = a.coords + i * a.ldc;
    float xi[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < a.sd) xi[k] = ci[k];
    for (int e = beg + lane; e < end; e += 64) {
      const unsigned lc = (unsigned)a.colidx[e] - cbase;
      float len = INFINITY;                    // out-of-block entries are never followed
      if (lc < n) len = gp_dist(xi, a.coords + (long long)(cbase + lc) * a.ldc, a.sd);
      if (e < a.nnz_cap) a.lens[e] = len;
    }
  }
}

__global__ void __launch_bounds__(kGpCompThreads) gp_components_kernel(GraphPathsArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];   // [n] labels, [n] sizes
  __shared__ unsigned sRed[2];
  int* sLab = reinterpret_cast<int*>(sRaw);
  int* sCnt = sLab + a.n;
  const int tid = threadIdx.x, nt = blockDim.x, n = a.n, g = blockIdx.x;
  const unsigned cbase = (unsigned)g * (unsigned)n;
  const int* rp = a.rowptr + (long long)g * n;

  for (int i = tid; i < n; i += nt) sLab[i] = i;
  if (tid < 2) sRed[tid] = 0u;
  __syncthreads();

  int any;
  do {
    int changed = 0;
    for (int i = tid; i < n; i += nt) {            // hook, both ways along the arc
      const int end = rp[i + 1];
      for (int e = rp[i]; e < end; ++e) {
        const unsigned lc = (unsigned)a.colidx[e] - cbase;
        if (lc >= (unsigned)n || lc == (unsigned)i) continue;
        const int li = sLab[i], lj = sLab[lc];
        if (li < lj) {
          atomicMin(&sLab[lj], li);
          atomicMin(&sLab[lc], li);
          changed = 1;
        } else if (lj < li) {
          atomicMin(&sLab[li], lj);
          atomicMin(&sLab[i], lj);
          changed = 1;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {            // follow the chain (it descends)
      const int l0 = sLab[i];
      int l = l0, ll;
      while ((ll = sLab[l]) != l) l = ll;
      if (l != l0) {
        atomicMin(&sLab[i], l);
        changed = 1;
      }
    }
    any = __syncthreads_or(changed);
  } while (any);

  for (int i = tid; i < n; i += nt) sCnt[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += nt) atomicAdd(&sCnt[sLab[i]], 1);
  __syncthreads();
  unsigned roots = 0, big = 0;
  for (int i = tid; i < n; i += nt) {
    roots += sLab[i] == i ? 1u : 0u;
    big = max(big, (unsigned)sCnt[i]);
    if (a.comp) a.comp[(long long)cbase + i] = sLab[i];
  }
  roots = wave_sum_u(roots);
  big = wave_max_u(big);
  if ((tid & 63) == 0) {
    atomicAdd(&sRed[0], roots);
    atomicMax(&sRed[1], big);
  }
  __syncthreads();
  if (tid < 2) a.totals[(long long)g * 6 + tid] = sRed[tid];
}

// One load step of a BFS row: the lanes holding an unseen in-block column claim it, the
// winners append it to the queue.  Returns the new queue length (wave-uniform).
__device__ __forceinline__ int gp_visit(unsigned short* sHop, unsigned short* sQ, unsigned lc, unsigned n,
                                        unsigned u, unsigned hnew, int qlen, int lane) {
  const bool cand = lc < n && lc != u && sHop[lc] == kGpUnseen;
  if (__ballot(cand) == 0ull) return qlen;
  const unsigned short mark = (unsigned short)(kGpMark | (unsigned)lane);
  if (cand) sHop[lc] = mark;
  gp_wave_sync();
  const bool win = cand && sHop[lc] == mark;
  const unsigned long long m = __ballot(win);
  gp_wave_sync();                               // every lane has read the marks
  if (win) {
    const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    sQ[qlen + (int)before] = (unsigned short)lc;
    sHop[lc] = (unsigned short)hnew;
  }
  gp_wave_sync();
  return qlen + __popcll(m);
}

// One load step of a relaxation: d[lc] = min(d[lc], fl(du + w)) on the bit patterns.
__device__ __forceinline__ bool gp_relax(unsigned* sDist, unsigned lc, unsigned n, unsigned u, float du, float w) {
  if (lc >= n || lc == u) return false;
  const unsigned cb = __float_as_uint(__fadd_rn(du, w));
  return cb < atomicMin(&sDist[lc], cb);
}

template <bool kRoutes>
__global__ void __launch_bounds__(64 * kGpWaves) gp_paths_kernel(GraphPathsArgs a) {
  // [2][256] histograms, [kGpWaves][4] wave totals, then per wave: hops [n], queue [n] (16-bit),
  // routes [n] (32-bit, with coords)
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];
  unsigned* sHist = reinterpret_cast<unsigned*>(sRaw);
  unsigned long long* sTot = reinterpret_cast<unsigned long long*>(sRaw + 2 * kGpBins * 4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nthreads = 64 * a.waves;
  const unsigned n = (unsigned)a.n;
  unsigned char* mine = sRaw + kGpFixedLds + (size_t)wave * n * (kRoutes ? 8 : 4);
  unsigned short* sHop = reinterpret_cast<unsigned short*>(mine);
  unsigned short* sQ = sHop + n;
  unsigned* sDist = reinterpret_cast<unsigned*>(mine + (size_t)n * 4);

  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  const unsigned cbase = (unsigned)g * n;
  const int* rp = a.rowptr + (long long)g * a.n;

  for (int i = tid; i < 2 * kGpBins; i += nthreads) sHist[i] = 0u;
  __syncthreads();

  unsigned long long tPairs = 0, tHops = 0;    // the wave's totals (wave-uniform)
  unsigned tMax = 0, tSrc = 0;

  for (int si = blk * a.waves + wave; si < a.n_src; si += a.bpg * a.waves) {
    const unsigned s = (unsigned)si * (unsigned)a.src_step;
    for (unsigned v = lane; v < n; v += 64) {
      sHop[v] = (unsigned short)kGpUnseen;
      if (kRoutes) sDist[v] = kGpInf;
    }
    gp_wave_sync();
    if (lane == 0) {
      sHop[s] = 0;
      sQ[0] = (unsigned short)s;
      if (kRoutes) sDist[s] = 0u;
    }
    gp_wave_sync();

    // ---- BFS: 64 queued nodes per batch, a lane each for their row bounds
    int qlen = 1;
    for (int head = 0, cnt = 0; head < qlen; head += cnt) {   // the queue grows while it is read
      cnt = min(64, qlen - head);
      int ul = 0, bl = 0, el = 0, hl = 0;      // lanes past cnt hold an empty row
      if (lane < cnt) {
        ul = sQ[head + lane];
        bl = rp[ul];
        el = rp[ul + 1];
        hl = sHop[ul];
      }
      for (int k = 0; k < cnt; k += 4) {       // k + 3 <= 63
        unsigned uu[4], hh[4], cc[4];
        int b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          uu[u] = (unsigned)__builtin_amdgcn_readlane(ul, k + u);
          hh[u] = (unsigned)__builtin_amdgcn_readlane(hl, k + u);
          b0[u] = __builtin_amdgcn_readlane(bl, k + u);
          b1[u] = __builtin_amdgcn_readlane(el, k + u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          cc[u] = ~0u;
          if (b0[u] + lane < b1[u]) cc[u] = (unsigned)a.colidx[b0[u] + lane] - cbase;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          qlen = gp_visit(sHop, sQ, cc[u], n, uu[u], hh[u] + 1u, qlen, lane);
          for (int e0 = b0[u] + 64; e0 < b1[u]; e0 += 64) {     // rows longer than one load
            unsigned lc = ~0u;
            if (e0 + lane < b1[u]) lc = (unsigned)a.colidx[e0 + lane] - cbase;
            qlen = gp_visit(sHop, sQ, lc, n, uu[u], hh[u] + 1u, qlen, lane);
          }
        }
      }
    }

    // ---- routes: sweeps over the queue until one lowers nothing
    if (kRoutes) {
      bool again;
      do {
        bool changed = false;
        for (int head = 0; head < qlen; head += 64) {
          const int cnt = min(64, qlen - head);
          int ul = 0, bl = 0, el = 0;
          if (lane < cnt) {
            ul = sQ[head + lane];
            bl = rp[ul];
            el = rp[ul + 1];
          }
          for (int k = 0; k < cnt; k += 4) {
            unsigned uu[4], cc[4];
            int b0[4], b1[4];
            float ww[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              uu[u] = (unsigned)__builtin_amdgcn_readlane(ul, k + u);
              b0[u] = __builtin_amdgcn_readlane(bl, k + u);
              b1[u] = __builtin_amdgcn_readlane(el, k + u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int e = b0[u] + lane;
              cc[u] = ~0u;
              ww[u] = INFINITY;
              if (e < b1[u]) {
                cc[u] = (unsigned)a.colidx[e] - cbase;
                if (e < a.nnz_cap) ww[u] = a.lens[e];
              }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float du = __uint_as_float(
                  __hip_atomic_load(&sDist[uu[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
              changed |= gp_relax(sDist, cc[u], n, uu[u], du, ww[u]);
              for (int e0 = b0[u] + 64; e0 < b1[u]; e0 += 64) {
                const int e = e0 + lane;
                unsigned lc = ~0u;
                float w = INFINITY;
                if (e < b1[u]) {
                  lc = (unsigned)a.colidx[e] - cbase;
                  if (e < a.nnz_cap) w = a.lens[e];
                }
                changed |= gp_relax(sDist, lc, n, uu[u], du, w);
              }
            }
          }
        }
        gp_wave_sync();
        again = __ballot(changed) != 0ull;
      } while (again);
    }

    // ---- epilogue: bins, totals and the optional per-source rows
    const long long orow = ((long long)g * a.n_src + si) * a.n;
    float xs[3] = {0.f, 0.f, 0.f};
    if (kRoutes) {
      const float* cs = a.coords + (long long)(cbase + s) * a.ldc;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < a.sd) xs[k] = cs[k];
    }
    unsigned pairs = 0, hsum = 0, hmax = 0;
    for (unsigned t = lane; t < n; t += 64) {
      const unsigned h = sHop[t];
      float r = INFINITY;
      if (kRoutes) r = __uint_as_float(sDist[t]);
      if (a.hops_out) a.hops_out[orow + t] = h == kGpUnseen ? -1 : (int)h;
      if (kRoutes && a.route_out) a.route_out[orow + t] = r;
      if (h != kGpUnseen && t != s) {
        ++pairs;
        hsum += h;
        hmax = max(hmax, h);
        atomicAdd(&sHist[min(h, (unsigned)kGpBins - 1u)], 1u);
        if (kRoutes) {
          const float e = gp_dist(xs, a.coords + (long long)(cbase + t) * a.ldc, a.sd);
          if (e > 0.f) atomicAdd(&sHist[kGpBins + gp_detour_bin(r, e, a.detour_scale)], 1u);
        }
      }
    }
    tPairs += wave_sum_u(pairs);
    tHops += wave_sum_u(hsum);
    tMax = max(tMax, wave_max_u(hmax));
    ++tSrc;
    gp_wave_sync();                             // the arrays are read; the next source clears them
  }

  if (lane == 0) {
    sTot[wave * 4 + 0] = tSrc;
    sTot[wave * 4 + 1] = tPairs;
    sTot[wave * 4 + 2] = tHops;
    sTot[wave * 4 + 3] = tMax;
  }
  __syncthreads();
  unsigned long long* hg = a.hist + (long long)g * 2 * kGpBins;
  for (int i = tid; i < 2 * kGpBins; i += nthreads) {
    const unsigned v = sHist[i];
    if (v) atomicAdd(&hg[i], (unsigned long long)v);
  }
  if (tid < 4) {
    unsigned long long v = 0;
    for (int w = 0; w < a.waves; ++w) v = tid < 3 ? v + sTot[w * 4 + tid] : max(v, sTot[w * 4 + tid]);
    if (v) {
      if (tid < 3) atomicAdd(&a.totals[(long long)g * 6 + 2 + tid], v);
      else atomicMax(&a.totals[(long long)g * 6 + 5], v);
    }
  }
}

// Workgroups per graph of gp_paths_kernel: sixteen per compute unit over the batch, never
// more than the graph has groups of sources.  Integer sums and maxima: the result does not
// depend on the choice.
static int graph_paths_blocks_per_graph(int ngraphs, int n_src, int waves) {
  const long long groups = ((long long)n_src + waves - 1) / waves;
  long long want = (16LL * device_cu_count() + ngraphs - 1) / ngraphs;
  if (want < 1) want = 1;
  if (want > groups) want = groups;
  return (int)want;
}

// The kernels take up to 8 n bytes (128 KiB at n = 16384) of dynamic LDS beside their fixed part.
static int graph_paths_allow_lds() {
  static std::once_flag once;
  static bool ok = true;
  std::call_once(once, [] {
    const int cap = kGpFixedLds + kGpMaxN * 8;
    ok = hipFuncSetAttribute(reinterpret_cast<const void*>(gp_paths_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, cap) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(gp_paths_kernel<false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, cap) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(gp_components_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, kGpMaxN * 8) == hipSuccess;
  });
  if (!ok) {
    set_error("snd_graph_paths: hipFuncSetAttribute failed");
    return SND_ERR_HIP;
  }
  return 0;
}

int launch_graph_paths(const GraphPathsArgs& a, hipStream_t s) {
  const long long blocks = (long long)a.bpg * a.ngraphs;
  SND_CHECK_ARG(a.bpg >= 1 && blocks < (1LL << 31), "snd_graph_paths: %lld workgroups", blocks);
  SND_TRY(graph_paths_allow_lds());
  if (hipMemsetAsync(a.hist, 0, (size_t)a.ngraphs * 2 * kGpBins * 8, s) != hipSuccess ||
      hipMemsetAsync(a.totals, 0, (size_t)a.ngraphs * 6 * 8, s) != hipSuccess) {
    set_error("snd_graph_paths: memset failed");
    return SND_ERR_HIP;
  }
  const bool routes = a.coords != nullptr;
  if (routes) {
    const long long rows = (long long)a.n * a.ngraphs;
    const long long want = (rows + 3) / 4, most = 64LL * device_cu_count();
    hipLaunchKernelGGL(gp_edge_len_kernel, dim3((unsigned)(want < most ? want : most)), dim3(256), 0, s, a);
    SND_LAUNCH_CHECK("gp_edge_len_kernel");
  }
  const int cthreads = (int)(round_up(a.n, 64) < kGpCompThreads ? round_up(a.n, 64) : kGpCompThreads);
  hipLaunchKernelGGL(gp_components_kernel, dim3((unsigned)a.ngraphs), dim3(cthreads), (size_t)a.n * 8, s, a);
  SND_LAUNCH_CHECK("gp_components_kernel");
  const size_t lds = kGpFixedLds + (size_t)a.waves * graph_paths_wave_lds(a.n, routes);
  if (routes)
    hipLaunchKernelGGL(gp_paths_kernel<true>, dim3((unsigned)blocks), dim3(64 * a.waves), lds, s, a);
  else
    hipLaunchKernelGGL(gp_paths_kernel<false>, dim3((unsigned)blocks), dim3(64 * a.waves), lds, s, a);
  SND_LAUNCH_CHECK("gp_paths_kernel");
  return 0;
}

}  // namespace snd

extern "C" size_t snd_graph_paths_workspace(int n_graphs, int n, long long nnz_cap, int has_coords) {
  if (n_graphs < 1 || n < 1 || n > snd::kGpMaxN || nnz_cap < 0 || !has_coords) return 0;
  return (size_t)snd::round_up((nnz_cap > 0 ? nnz_cap : 1) * 4, 16);   // one fp32 length per entry
}

extern "C" int snd_graph_paths(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                               const float* coords, int ldc, int sd, float detour_scale, int src_step,
                               int* comp, int* hops_out, float* route_out, long long* hist,
                               long long* totals, void* workspace, size_t workspace_bytes,
                               snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(rowptr && hist && totals, "snd_graph_paths: null operand");
  SND_CHECK_ARG(n_graphs >= 1 && n >= 1, "snd_graph_paths: empty batch");
  SND_CHECK_ARG(n <= kGpMaxN, "snd_graph_paths: n=%d > %d (hop counts are 16-bit on chip)", n, kGpMaxN);
  SND_CHECK_ARG((long long)n * n_graphs < (1LL << 31), "snd_graph_paths: n=%d x %d graphs too large", n,
                n_graphs);
  SND_CHECK_ARG(src_step >= 1, "snd_graph_paths: src_step=%d < 1", src_step);
  SND_CHECK_ARG(nnz_cap >= 0 && (colidx || nnz_cap == 0), "snd_graph_paths: colidx of %lld entries", nnz_cap);
  SND_CHECK_ARG(coords || !route_out, "snd_graph_paths: route_out needs coords");
  if (coords) {
    SND_CHECK_ARG(sd >= 1 && sd <= 3, "snd_graph_paths: sd=%d not in [1, 3]", sd);
    SND_CHECK_ARG(ldc >= sd, "snd_graph_paths: ldc=%d < sd=%d", ldc, sd);
    SND_CHECK_ARG(detour_scale > 0.f && std::isfinite(detour_scale),
                  "snd_graph_paths: detour_scale must be finite and > 0");
  }
  const size_t need = snd_graph_paths_workspace(n_graphs, n, nnz_cap, coords != nullptr);
  SND_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                "snd_graph_paths: workspace %zu < %zu", workspace_bytes, need);
  const int n_src = (int)(((long long)n + src_step - 1) / src_step);
  const int waves = graph_paths_waves(n, coords != nullptr);
  GraphPathsArgs a{rowptr, colidx, n, n_graphs, coords, ldc, sd, detour_scale, src_step, n_src,
                   comp, hops_out, route_out,
                   reinterpret_cast<unsigned long long*>(hist),
                   reinterpret_cast<unsigned long long*>(totals),
                   reinterpret_cast<float*>(workspace), nnz_cap, waves,
                   graph_paths_blocks_per_graph(n_graphs, n_src, waves)};
  return launch_graph_paths(a, (hipStream_t)stream);
}
