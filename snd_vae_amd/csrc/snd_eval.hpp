#pragma once
#include "snd_common.hpp"

namespace snd {

// Edge-score evaluation of the inner-product decoder (snd_zzt_eval): L = J J^T per graph on
// the fp32 matrix cores (v_mfma_f32_32x32x2_f32, k ascending from a zero accumulator: bit for
// bit the fmaf chain of gen_adj_kernel), every logit classified and binned on chip.
//
// Per graph b, over the n^2 - n ordered off-diagonal pairs:
//   hist[b][label][bin] += 1, label = 1 when (i, j) is a CSR entry, bin = clamp(floor(64 L)
//   + 1024, 0, 2047): 2048 bins of width 1/64 over [-16, 16), bins 0 and 2047 the under- and
//   overflow bins.  64 L is exact, so the bin is a pure function of the fp32 logit.
//   counts[b] = {TP, FP, FN, TN} at the decision rule L > 0 (model.py:208); the n diagonal
//   pairs are TN (model.py:185,205-207), so (TP + TN) / n^2 is main.py:334's accuracy.
//
// All sums are integer sums (32-bit LDS counters per workgroup, flushed with 64-bit global
// atomics), so the result does not depend on scheduling, on the column split or on the
// order the workgroups finish in: two runs on the same operands are bitwise equal.
constexpr int kEvalBins = 2048;

// The cell of a score (a zz^T logit, or the e2e decoder's margin in snd_margin_eval):
// label * 2048 + clamp(floor(64 L) + 1024, 0, 2047).  The clamp is done in float and once
// more on the integer, so no input (non-finite scores are unspecified, but must not fault)
// can address outside the histogram.
__device__ __forceinline__ unsigned eval_key(float L, unsigned label) {
  const float t = __builtin_amdgcn_fmed3f(floorf(L * 64.f) + 1024.f, 0.f, 2047.f);
  return (label << 11) | min((unsigned)t, (unsigned)kEvalBins - 1u);
}

struct ZztEvalArgs {
  const float* z; int ldz; int d;      // [B*n, ldz] fp32 decoder input J, 1 <= d <= 128
  int n, ngraphs;
  const int* rowptr;                   // [B*n + 1] block-diagonal CSR (as snd_zzt_ce)
  const int* colidx;                   // global column ids, any order within a row
  unsigned long long* hist;            // [B][2][kEvalBins]
  unsigned long long* counts;          // [B][4] = {TP, FP, FN, TN}
  int nsplit;                          // column splits per 128-row strip (zzt_eval_splits)
};

int zzt_eval_splits(int ngraphs, int n);
// accumulate == 0: hist and counts are cleared on the stream first
int launch_zzt_eval(const ZztEvalArgs& a, int accumulate, hipStream_t s);

}  // namespace snd
