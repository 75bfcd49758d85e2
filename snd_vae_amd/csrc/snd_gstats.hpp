#pragma once
#include "snd_common.hpp"

namespace snd {

// Graph statistics of a block-diagonal CSR (snd_graph_stats): per row the degree and
// tri2 = sum_{j in N(i)} |N(i) & N(j)|, per graph the degree / local-clustering / edge-length
// histograms and four totals, in one launch.  Integer results only.
constexpr int kGsBins = 256;
constexpr int kGsWaves = 4;          // waves per workgroup, one row in flight each
constexpr int kGsMaxN = 32768;       // tri2 <= (n - 1)(n - 2) fits int32

struct GraphStatsArgs {
  const int* rowptr;                 // [B*n + 1]
  const int* colidx;                 // global column ids, any order within a row
  int n, ngraphs;
  const float* coords;               // [B*n, ldc] or NULL (no edge-length histogram)
  int ldc, sd;                       // 1 <= sd <= 3
  float len_scale;                   // bins per unit of length
  int* deg;                          // [B*n] or NULL
  int* tri2;                         // [B*n] or NULL
  unsigned long long* hist;          // [B, 3, 256]
  unsigned long long* totals;        // [B, 4]
  int bpg;                           // workgroups per graph
  int words;                         // 32-bit words of one row mask: ceil(n / 32)
};

int graph_stats_blocks_per_graph(int ngraphs, int n);
int launch_graph_stats(const GraphStatsArgs& a, int accumulate, hipStream_t s);

}  // namespace snd
