#pragma once
#include "snd_common.hpp"

namespace snd {

// Chebyshev moments of the spectral density of the normalised Laplacian of every graph block of
// a block-diagonal CSR (snd_graph_spectrum).  fp64 state, weights and sums; integer atomics for
// the counts only; every floating-point sum has a fixed order.
constexpr int kGsMaxN = 16384;
constexpr int kGsMaxMoments = 512;
constexpr int kGsWidth = 32;         // probe columns per block: a state row is 256 B, half a wave
constexpr int kGsTileRows = 8;       // rows of a 256-thread workgroup of the global step kernel
constexpr int kGsLdsMaxN = 64;       // the one-launch LDS path holds both state buffers: 2 n 256 B
constexpr int kGsLdsBudget = 64 * 1024;
constexpr unsigned kGsPhiloxTag = 0x53504543u;   // "SPEC": the probes' own Philox stream

struct GraphSpectrumArgs {
  const int* rowptr;                 // [B*n + 1]
  const int* colidx;                 // global column ids, any order
  long long nnz_cap;                 // entries colidx and wgt hold
  int n, ngraphs;
  int n_moments, n_probes;           // n_probes = 0: the n unit vectors
  unsigned long long seed;
  double* moments;                   // [B, n_moments]; raw dot sums until gs_final_kernel
  long long* info;                   // [B, 4]
  unsigned long long* acc;           // workspace: [B, 4] {sum of degrees, isolated, one-way, -}
  double* wgt;                       // workspace: [nnz_cap] 1/sqrt(d_i d_j) of a mutual entry, else 0
  double* state;                     // workspace: two buffers [B*n, kGsWidth]
  double* slab;                      // workspace: [B, tiles, 2] partial dots of one step
  int* deg;                          // workspace: [B*n]
  int tiles;                         // row tiles per graph of the global step kernel
  int lds_cap;                       // CSR entries of one graph the LDS path stages
};

inline int graph_spectrum_tiles(int n) { return (n + kGsTileRows - 1) / kGsTileRows; }
// Recurrence steps for K moments: step s leaves mu_{2s+1} and mu_{2s+2}.
inline int graph_spectrum_steps(int n_moments) { return n_moments / 2; }
// Probe blocks of a call.
inline int graph_spectrum_blocks(int n, int n_probes) {
  return ((n_probes > 0 ? n_probes : n) + kGsWidth - 1) / kGsWidth;
}
// LDS of the one-launch path, bytes: both state buffers, the raw moments, two sets of per-wave
// partial dots, then per staged CSR entry a weight (8 B) and a local column (2 B), and n + 1 row
// offsets.  The entry capacity is what a simple graph needs, n (n - 1), cut to the budget.
inline size_t graph_spectrum_lds_fixed(int n, int n_moments) {
  return (size_t)2 * n * kGsWidth * 8 + (size_t)n_moments * 8 + 16 * 8 + (((size_t)n + 2) / 2) * 8;
}
inline int graph_spectrum_lds_cap(int n, int n_moments) {
  const long long room = ((long long)kGsLdsBudget - (long long)graph_spectrum_lds_fixed(n, n_moments)) / 10;
  long long want = (long long)n * (n - 1);
  if (want < 16) want = 16;
  const long long cap = (want < room ? want : room) & ~3LL;
  return (int)(cap > 0 ? cap : 0);
}
inline size_t graph_spectrum_lds_bytes(int n, int n_moments) {
  return graph_spectrum_lds_fixed(n, n_moments) + (size_t)graph_spectrum_lds_cap(n, n_moments) * 10;
}
int launch_graph_spectrum(const GraphSpectrumArgs& a, bool use_lds, hipStream_t s);

}  // namespace snd
