#pragma once
#include "snd_common.hpp"

namespace snd {

// Edge crossings of a block-diagonal CSR drawn at its nodes' coordinates (snd_graph_crossings):
// per graph the crossing pairs of the mutual-edge graph's edges under the exact predicate of
// include/snd_vae.h, per-edge crossing counts, the orientation histogram and the crossing-angle
// histogram.  Integer atomics only.
constexpr int kGxMaxN = 16384;       // local ids are packed two to a 32-bit word
constexpr int kGxTile = 64;          // edges per tile: a lane holds one e-edge, a wave stages 64 f-edges
constexpr int kGxOwnScan = 64;      // gx_prep_kernel: a row this short is searched by one lane
constexpr int kGxWaves = 4;          // waves per workgroup; every wave walks its own work items
constexpr int kGxGridPerCu = 8;       // four-wave workgroups of gx_pairs_kernel per compute unit (five are resident)
constexpr int kGxAcc = 8;            // 64-bit accumulators per graph in the workspace
constexpr int kGxCounts = 7;
constexpr int kGxBins = 256;

enum { GX_E = 0,      // edges (a < b), also the append cursor of the edge list
       GX_X,          // crossing pairs
       GX_CROSSED,    // edges with >= 1 crossing
       GX_W,          // sum_v C(deg_v, 2): the pairs of edges that share a node
       GX_ONEWAY,     // arcs i -> j of the CSR without j -> i
       GX_ZERO,       // edges whose endpoints coincide
       GX_MAXC };     // largest crossing count of one edge

struct GraphCrossingsArgs {
  const int* rowptr;                 // [B*n + 1]
  const int* colidx;                 // global column ids, any order
  long long nnz_cap;                 // entries colidx and every edge array hold
  int n, ngraphs;
  const float* coords;               // [B*n, ldc], columns 0 and 1
  int ldc;
  long long work_cap;
  long long* counts;                 // [B, 7]
  long long* hist;                   // [B, 3, 256]
  unsigned long long* work;          // [B]
  int* cross_out;                    // [nnz_cap] or NULL
  unsigned long long* acc;           // workspace: [B, kGxAcc]
  long long* item_prefix;            // workspace: [B + 1] exclusive prefix of the per-graph tile pairs
  float4* ept;                       // workspace: edge list, (ax, ay, bx, by); graph g's edges at
  unsigned* eab;                     //   rowptr[g n] .. + E_g;  a | b << 16 (local ids, a < b)
  int* epos;                         //   CSR position of the entry (row a, column b)
  unsigned* ecnt;                    //   crossing count of the edge
  int words;                         // 32-bit words of an n-bit mask
  int pair_blocks;                   // workgroups of gx_pairs_kernel
  int bpg;                           // workgroups per graph of gx_finish_kernel
};

int launch_graph_crossings(const GraphCrossingsArgs& a, hipStream_t s);

}  // namespace snd
