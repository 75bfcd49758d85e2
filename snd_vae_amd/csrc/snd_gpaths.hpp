#pragma once
#include "snd_common.hpp"

namespace snd {

// Path statistics of a block-diagonal CSR (snd_graph_paths): weak components per graph,
// BFS hop counts and fp32 shortest routes from a set of sources, their histograms and six
// totals.  Integer atomics only.
constexpr int kGpBins = 256;
constexpr int kGpMaxN = 16384;       // hop counts, queue entries and claim marks are 16-bit
constexpr int kGpWaves = 4;          // waves per workgroup of gp_paths_kernel while four fit
constexpr int kGpCompThreads = 1024;
// fixed LDS of gp_paths_kernel: [2][256] 32-bit histograms, [kGpWaves][4] 64-bit wave totals
constexpr int kGpFixedLds = 2 * kGpBins * 4 + kGpWaves * 4 * 8;
constexpr int kGpSmallLds = 64 * 1024;   // four waves per workgroup while they fit in this

struct GraphPathsArgs {
  const int* rowptr;                 // [B*n + 1]
  const int* colidx;                 // global column ids, any order, duplicates allowed
  int n, ngraphs;
  const float* coords;               // [B*n, ldc] or NULL (no routes, no detour histogram)
  int ldc, sd;                       // 1 <= sd <= 3
  float detour_scale;                // bins per unit of (route / straight line - 1)
  int src_step, n_src;               // sources 0, src_step, ...; n_src = ceil(n / src_step)
  int* comp;                         // [B*n] or NULL
  int* hops_out;                     // [B*n_src, n] or NULL
  float* route_out;                  // [B*n_src, n] or NULL (needs coords)
  unsigned long long* hist;          // [B, 2, 256]
  unsigned long long* totals;        // [B, 6]
  float* lens;                       // workspace: one length per CSR entry (coords only)
  long long nnz_cap;                 // entries the workspace holds
  int waves;                         // waves per workgroup of gp_paths_kernel: kGpWaves or 1
  int bpg;                           // its workgroups per graph
};

// Bytes of one wave's arrays in gp_paths_kernel: hops and queue (16-bit each), routes (fp32).
inline size_t graph_paths_wave_lds(int n, bool coords) { return (size_t)n * (coords ? 8 : 4); }
// Four waves per workgroup while four sets of arrays fit in 64 KiB, one wave above that:
// n <= 1980 with coords, n <= 3960 without.
inline int graph_paths_waves(int n, bool coords) {
  return kGpFixedLds + kGpWaves * graph_paths_wave_lds(n, coords) <= (size_t)kGpSmallLds ? kGpWaves : 1;
}
int launch_graph_paths(const GraphPathsArgs& a, hipStream_t s);

}  // namespace snd
