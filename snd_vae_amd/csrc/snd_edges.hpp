#pragma once
#include "snd_common.hpp"

namespace snd {

// Edge extraction of the inner-product decoder (snd_zzt_edges): L = J J^T per graph on the
// fp32 matrix cores (the tile body of zzt_eval_kernel, snd_zzt_tile.hpp: bit for bit the fmaf
// chain of gen_adj_kernel), thresholded on chip, the predicted graph written as the
// block-diagonal CSR with ascending global column ids.  Three stream-ordered launches:
//   count  every workgroup (a 128-row strip x a contiguous range of 128-column tiles, as
//          zzt_eval_kernel) writes its rows' hit counts to cnt[graph][split][row];
//   scan   one workgroup: row totals over the splits, the exclusive scan into rowptr, the
//          int64 total into *nnz, every cnt cell replaced by the start of its segment;
//   fill   the count pass's grid recomputes L and emits each row's hits in ascending column
//          order from the segment start.  Every workgroup reads the total and leaves when it
//          does not fit the capacity.
// Integer results only: independent of scheduling and of the column split.
struct ZztEdgesArgs {
  const float* z; int ldz; int d;      // [B*n, ldz] fp32 decoder input J, 1 <= d <= 128
  int n, ngraphs;
  float threshold; int inclusive;      // edge iff i != j and L > threshold (>= when inclusive)
  int* rowptr;                         // [B*n + 1]
  int* colidx;                         // [cap] or NULL (count and scan only)
  long long cap;
  long long* nnz;                      // device int64: the exact total
  int* cnt;                            // workspace [B][nsplit][n]
  int nsplit;                          // column splits per 128-row strip (zzt_eval_splits)
};

size_t zzt_edges_workspace(int ngraphs, int n, int nsplit);
int launch_zzt_edges(const ZztEdgesArgs& a, hipStream_t s);

}  // namespace snd
