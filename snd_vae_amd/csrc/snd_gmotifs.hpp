#pragma once
#include "snd_common.hpp"

namespace snd {

// Graphlet census of a block-diagonal CSR (snd_graph_motifs): the nine induced 2- to 4-node
// subgraph counts of the mutual-edge graph of every graph block, the one-way arc count and
// the work bound that gates the counting.  Integer arithmetic and integer atomics only.
constexpr int kGmMaxN = 16384;       // local ids are kept in 16 bits on chip (lists, counters)
constexpr int kGmWaves = 4;          // waves per workgroup while four sets of arrays fit
constexpr int kGmSmallLds = 64 * 1024;
constexpr int kGmAcc = 10;           // 64-bit accumulators per graph in the workspace
constexpr int kGmCensus = 10;

// the accumulators (raw sums; gm_final_kernel converts them to induced counts)
enum { GM_SUMD = 0,   // sum_v d_v = 2E
       GM_W,          // sum_v C(d_v, 2)
       GM_S3P,        // sum_v C(d_v, 3)
       GM_ONEWAY,     // arcs i -> j of the CSR without j -> i
       GM_T6,         // sum_u sum_{v in N(u)} t(u, v) = 6T
       GM_TT2,        // sum_u (sum_{v in N(u)} t(u, v)) (d_u - 2) = 2TT'
       GM_DP,         // sum_{uv in E} C(t(u, v), 2) = D'
       GM_PSUM,       // sum_{uv in E} (d_u - 1)(d_v - 1)
       GM_C4P2,       // sum_{u < w} C(c(u, w), 2) = 2C4'
       GM_K4 };

struct GraphMotifsArgs {
  const int* rowptr;                 // [B*n + 1]
  const int* colidx;                 // global column ids, any order
  long long nnz_cap;                 // entries colidx and mcol hold
  int n, ngraphs;
  long long work_cap;
  long long* census;                 // [B, 10]
  unsigned long long* work;          // [B]
  unsigned long long* acc;           // workspace: [B, kGmAcc]
  int* deg;                          // workspace: [B*n] degrees of the mutual-edge graph
  int* mcol;                         // workspace: row i of the mutual-edge CSR, local ids, at
                                     //   rowptr[i] .. rowptr[i] + deg[i]
  int words;                         // 32-bit words of an n-bit mask
  int waves;                         // waves per workgroup of the three counting kernels
  int bpg;                           // their workgroups per graph
};

// LDS of one wave in the counting kernels, the largest of the three layouts (gm_clique_kernel:
// two n-bit masks and a list of n 16-bit ids; gm_wedge_kernel: one mask and n 16-bit counters).
inline size_t graph_motifs_wave_lds(int n) {
  const size_t words = ((size_t)n + 31) / 32, halves = ((size_t)n + 1) / 2;
  return (2 * words + halves) * 4;
}
// Four waves per workgroup while four sets of arrays fit in 64 KiB (n <= 7280), one wave
// above that (36 KiB at n = 16384: four workgroups per CU).
inline int graph_motifs_waves(int n) {
  return kGmWaves * graph_motifs_wave_lds(n) <= (size_t)kGmSmallLds ? kGmWaves : 1;
}
int launch_graph_motifs(const GraphMotifsArgs& a, hipStream_t s);

}  // namespace snd
