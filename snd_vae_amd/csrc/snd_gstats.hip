// Graph statistics of a block-diagonal CSR (snd_graph_stats): degree, triangles, local
// clustering and edge length of B graphs x n nodes in one launch, from the CSR that
// DeviceBatch holds or snd_zzt_edges writes, and the node coordinates.
//
// N(i) is the set of columns of row i inside i's graph block, i itself left out.  A wave owns
// a row i: it sets N(i) as an n-bit mask in LDS (512 B at n = 4096, 2 KB at 16384; four waves
// per workgroup, each with a mask of its own), then walks the neighbours j in groups of four;
// its lanes stride over row j's colidx with coalesced loads and test every entry against the
// mask.  deg[i] = |N(i)|, tri2[i] = sum_j |N(i) & N(j)| (twice the triangles at i on a
// symmetric CSR).  The same walk bins the length of every entry with column > row.
//
// Work: sum_j deg(j)^2 entries tested, the wedge count of the graph; bytes: the same number
// of 4-byte column ids (from L2 for the graphs this project generates), plus one pass over
// the CSR and the gathered coordinate rows.
//
// Rows of a graph are dealt round-robin over the graph's waves (row = first + k * waves): the
// rows of a hub and of its neighbourhood, adjacent in a locality-ordered batch, land on
// different waves and workgroups.  A hub row of degree D still runs on one wave for D walks
// of ceil(deg(j) / 64) load steps each; nothing splits a row, so the longest row bounds the
// tail of the launch while every other wave keeps taking its own rows.
//
// The three histograms live per workgroup in LDS (32-bit integer atomics); the non-zero bins
// and the totals are flushed to the int64 outputs with 64-bit vector atomics, as
// zzt_eval_kernel flushes.  Integer sums only: two runs are bitwise equal.
#include "snd_gstats.hpp"

#include <cmath>

namespace snd {

// Is local column lc of row j's entries a member of the masked N(i)?  Out-of-block entries
// (lc >= n as unsigned) and row j's self loop are no members of N(j).
__device__ __forceinline__ unsigned gs_hit(const unsigned* sMask, unsigned lc, unsigned n, unsigned j) {
  if (lc >= n || lc == j) return 0u;
  return (sMask[lc >> 5] >> (lc & 31u)) & 1u;
}

// The bin of an edge length: min(floor(len * scale), 255).  The clamp is done in float and
// once more on the integer, so no coordinate (non-finite ones are unspecified, but must not
// fault) can address outside the histogram.
__device__ __forceinline__ unsigned gs_len_bin(float len, float scale) {
  const float t = fminf(fmaxf(floorf(len * scale), 0.f), (float)(kGsBins - 1));
  return min((unsigned)t, (unsigned)kGsBins - 1u);
}

__global__ void __launch_bounds__(64 * kGsWaves) graph_stats_kernel(GraphStatsArgs a) {
  // [kGsWaves][4] wave totals, [3][256] histograms, [kGsWaves][words] row masks
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];
  unsigned long long* sTot = reinterpret_cast<unsigned long long*>(sRaw);
  unsigned* sHist = reinterpret_cast<unsigned*>(sRaw + kGsWaves * 4 * 8);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* sMask = sHist + 3 * kGsBins + wave * a.words;

  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  const unsigned n = (unsigned)a.n;
  const unsigned cbase = (unsigned)g * n;
  const int* rp = a.rowptr + (long long)g * a.n;
  const bool lens = a.coords != nullptr;

  for (int i = tid; i < 3 * kGsBins; i += 64 * kGsWaves) sHist[i] = 0u;
  for (int w = lane; w < a.words; w += 64) sMask[w] = 0u;
  __syncthreads();

  unsigned long long tDeg = 0, tTri = 0, tDd = 0, tEdge = 0;   // the wave's totals (wave-uniform)

  for (int li = blk * kGsWaves + wave; li < a.n; li += a.bpg * kGsWaves) {
    const int beg = rp[li], end = rp[li + 1];

    // N(i) into the mask
    unsigned dcnt = 0;
    for (int e0 = beg; e0 < end; e0 += 64) {
      const int e = e0 + lane;
      unsigned lc = ~0u;
      if (e < end) lc = (unsigned)a.colidx[e] - cbase;
      if (lc < n && lc != (unsigned)li) {
        atomicOr(&sMask[lc >> 5], 1u << (lc & 31u));
        ++dcnt;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the mask is complete
    __builtin_amdgcn_wave_barrier();

    float xi[3] = {0.f, 0.f, 0.f};
    if (lens) {
      const float* ci = a.coords + (long long)(cbase + (unsigned)li) * a.ldc;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < a.sd) xi[k] = ci[k];
    }

    // the walk: 64 neighbours per pass, one per lane; four rows j in flight
    unsigned tcnt = 0, ecnt = 0;
    for (int e0 = beg; e0 < end; e0 += 64) {
      const int e = e0 + lane;
      unsigned lc = ~0u;
      if (e < end) lc = (unsigned)a.colidx[e] - cbase;
      const bool ok = lc < n && lc != (unsigned)li;
      int jb = 0, je = 0;
      if (ok) {
        jb = rp[lc];
        je = rp[lc + 1];
      } else {
        lc = ~0u;
      }
      if (ok && lc > (unsigned)li) {          // one count per entry with column > row
        ++ecnt;
        if (lens) {
          const float* cj = a.coords + (long long)(cbase + lc) * a.ldc;
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (k < a.sd) {
              const float d = xi[k] - cj[k];
              s += d * d;
            }
          }
          atomicAdd(&sHist[2 * kGsBins + gs_len_bin(sqrtf(s), a.len_scale)], 1u);
        }
      }
      const int cnt = min(64, end - e0);
      for (int k = 0; k < cnt; k += 4) {      // k + 3 <= 63; lanes past cnt hold an empty row
        unsigned jj[4], cc[4];
        int b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          jj[u] = (unsigned)__builtin_amdgcn_readlane((int)lc, k + u);
          b0[u] = __builtin_amdgcn_readlane(jb, k + u);
          b1[u] = __builtin_amdgcn_readlane(je, k + u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          cc[u] = ~0u;
          if (b0[u] + lane < b1[u]) cc[u] = (unsigned)a.colidx[b0[u] + lane] - cbase;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) tcnt += gs_hit(sMask, cc[u], n, jj[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {         // rows j longer than one wave load
          for (int ee = b0[u] + 64 + lane; ee < b1[u]; ee += 64)
            tcnt += gs_hit(sMask, (unsigned)a.colidx[ee] - cbase, n, jj[u]);
        }
      }
    }

    const unsigned deg = wave_sum_u(dcnt), tri = wave_sum_u(tcnt), edges = wave_sum_u(ecnt);
    const unsigned long long dd = (unsigned long long)deg * (deg ? deg - 1u : 0u);
    tDeg += deg;
    tTri += tri;
    tDd += dd;
    tEdge += edges;
    if (lane == 0) {
      const long long row = (long long)cbase + li;
      if (a.deg) a.deg[row] = (int)deg;
      if (a.tri2) a.tri2[row] = (int)tri;
      atomicAdd(&sHist[min(deg, (unsigned)kGsBins - 1u)], 1u);
      unsigned long long cb = 0;               // deg < 2: c = 0
      if (deg >= 2u) cb = min(256ull * tri / dd, (unsigned long long)kGsBins - 1ull);
      atomicAdd(&sHist[kGsBins + (unsigned)cb], 1u);
    }

    __builtin_amdgcn_wave_barrier();           // every lane's mask reads are done
    for (int w = lane; w < a.words; w += 64) sMask[w] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  if (lane == 0) {
    sTot[wave * 4 + 0] = tDeg;
    sTot[wave * 4 + 1] = tTri;
    sTot[wave * 4 + 2] = tDd;
    sTot[wave * 4 + 3] = tEdge;
  }
  __syncthreads();
  unsigned long long* hg = a.hist + (long long)g * 3 * kGsBins;
  for (int i = tid; i < 3 * kGsBins; i += 64 * kGsWaves) {
    const unsigned v = sHist[i];
    if (v) atomicAdd(&hg[i], (unsigned long long)v);
  }
  if (tid < 4) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < kGsWaves; ++w) v += sTot[w * 4 + tid];
    if (v) atomicAdd(&a.totals[(long long)g * 4 + tid], v);
  }
}

// Workgroups per graph: eight per compute unit over the batch (the wave limit of a CU at
// four waves each), never more than the graph has groups of four rows.  The integer sums
// make the result independent of the choice.
int graph_stats_blocks_per_graph(int ngraphs, int n) {
  const long long groups = ((long long)n + kGsWaves - 1) / kGsWaves;
  long long want = (8LL * device_cu_count() + ngraphs - 1) / ngraphs;
  if (want < 1) want = 1;
  if (want > groups) want = groups;
  return (int)want;
}

int launch_graph_stats(const GraphStatsArgs& a, int accumulate, hipStream_t s) {
  const long long blocks = (long long)a.bpg * a.ngraphs;
  SND_CHECK_ARG(a.bpg >= 1 && blocks < (1LL << 31), "snd_graph_stats: %lld workgroups", blocks);
  if (!accumulate) {
    if (hipMemsetAsync(a.hist, 0, (size_t)a.ngraphs * 3 * kGsBins * 8, s) != hipSuccess ||
        hipMemsetAsync(a.totals, 0, (size_t)a.ngraphs * 4 * 8, s) != hipSuccess) {
      set_error("snd_graph_stats: memset failed");
      return SND_ERR_HIP;
    }
  }
  const size_t lds = (size_t)kGsWaves * 4 * 8 + (size_t)3 * kGsBins * 4 + (size_t)kGsWaves * a.words * 4;
  hipLaunchKernelGGL(graph_stats_kernel, dim3((unsigned)blocks), dim3(64 * kGsWaves), lds, s, a);
  SND_LAUNCH_CHECK("graph_stats_kernel");
  return 0;
}

}  // namespace snd

extern "C" size_t snd_graph_stats_workspace(int n_graphs, int n) {
  (void)n_graphs; (void)n;
  return 0;   // every partial sum lives in LDS
}

extern "C" int snd_graph_stats(const int* rowptr, const int* colidx, int n_graphs, int n,
                               const float* coords, int ldc, int sd, float len_scale,
                               int* deg, int* tri2, long long* hist, long long* totals,
                               int accumulate, void* workspace, size_t workspace_bytes,
                               snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(rowptr && hist && totals, "snd_graph_stats: null operand");
  SND_CHECK_ARG(n_graphs >= 1 && n >= 1, "snd_graph_stats: empty batch");
  SND_CHECK_ARG(n <= kGsMaxN, "snd_graph_stats: n=%d > %d (tri2 is int32)", n, kGsMaxN);
  SND_CHECK_ARG((long long)n * n_graphs < (1LL << 31), "snd_graph_stats: n=%d x %d graphs too large", n,
                n_graphs);
  if (coords) {
    SND_CHECK_ARG(sd >= 1 && sd <= 3, "snd_graph_stats: sd=%d not in [1, 3]", sd);
    SND_CHECK_ARG(ldc >= sd, "snd_graph_stats: ldc=%d < sd=%d", ldc, sd);
    SND_CHECK_ARG(len_scale >= 0.f && std::isfinite(len_scale),
                  "snd_graph_stats: len_scale must be finite and >= 0");
  }
  const size_t need = snd_graph_stats_workspace(n_graphs, n);
  SND_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                "snd_graph_stats: workspace %zu < %zu", workspace_bytes, need);
  // colidx may be NULL only for a CSR without entries; the kernel never reads it then
  GraphStatsArgs a{rowptr, colidx, n, n_graphs, coords, ldc, sd, len_scale, deg, tri2,
                   reinterpret_cast<unsigned long long*>(hist),
                   reinterpret_cast<unsigned long long*>(totals),
                   graph_stats_blocks_per_graph(n_graphs, n), (n + 31) / 32};
  return launch_graph_stats(a, accumulate, (hipStream_t)stream);
}
