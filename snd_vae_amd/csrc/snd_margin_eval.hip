// The disentangled model's loss tail and edge-score evaluation (ABI 23).
//
// snd_disent_losses: one thread turns the partial results a step's ops left on the device
// (snd_sigmoid_mse's sse blocks, snd_e2e_head_ce's {CE sum, correct}, snd_latent_reg's out[4]
// per group) into the eight loss terms, so the step reads nothing back.
//
// snd_margin_eval: snd_zzt_eval's histograms and confusion counts for the e2e structure
// decoder, whose edge score is the margin l1 - l0 that snd_e2e_decode writes.  The operands
// are dense, so the kernel is a stream over [B, N, N]: a workgroup owns one chunk of one
// graph's N^2 entries, bins them into an LDS histogram and flushes the non-zero bins.
#include "snd_eval.hpp"

namespace snd {
namespace {

struct DisentLossArgs {
  const double* sse_node; int node_blocks; double node_count;
  const double* sse_spatial; int spatial_blocks; double spatial_count;
  const double* ce_out; double pair_count;
  const double *reg_s, *reg_g, *reg_sg;
  double* losses;
};

__global__ void __launch_bounds__(64) disent_losses_kernel(DisentLossArgs a) {
  if (threadIdx.x != 0) return;
  double sn = 0.0, ss = 0.0;
  for (int i = 0; i < a.node_blocks; ++i) sn += a.sse_node[i];
  for (int i = 0; i < a.spatial_blocks; ++i) ss += a.sse_spatial[i];
  const double node_cost = sn / a.node_count;
  const double spatial_cost = ss / a.spatial_count;
  const double adj_cost = a.ce_out[0] / a.pair_count;
  double reg = 0.0;                       // disent.disentangled_cost: s, g, sg
  if (a.reg_s) reg += a.reg_s[1];
  if (a.reg_g) reg += a.reg_g[1];
  reg += a.reg_sg[1];
  a.losses[0] = adj_cost + node_cost + spatial_cost + reg;
  a.losses[1] = spatial_cost;
  a.losses[2] = adj_cost;
  a.losses[3] = node_cost;
  a.losses[4] = a.reg_g ? a.reg_g[0] : 0.0;
  a.losses[5] = a.reg_s ? a.reg_s[0] : 0.0;
  a.losses[6] = a.reg_sg[0];
  a.losses[7] = a.ce_out[1];
}

constexpr int kMeThreads = 256;
constexpr int kMeChunk = 8192;   // entries of one graph per workgroup: 8 trips of 256 x 4

// Entry e of a graph's row-major [N, N] block is on the diagonal iff e % (N + 1) == 0.  The
// callers keep r = e % (N + 1) per lane and pass r + k, k < 4: below 2 (N + 1) once
// N + 1 >= 4, so two compares decide; N = 1, 2 take the division.
__device__ __forceinline__ bool me_on_diag(unsigned rk, unsigned np1) {
  return np1 >= 4u ? (rk == 0u || rk == np1) : rk % np1 == 0u;
}

struct MeCounts { unsigned tp, fp, fn; };   // wave-uniform

// One entry per lane, every lane of the wave present (the ballots).
__device__ __forceinline__ void me_count(unsigned* sHist, float m, float a, bool valid, MeCounts& c) {
  const bool lab = a != 0.f, pred = m > 0.f;
  if (valid) atomicAdd(&sHist[eval_key(m, lab ? 1u : 0u)], 1u);
  c.tp += (unsigned)__popcll(__ballot(valid && lab && pred));
  c.fp += (unsigned)__popcll(__ballot(valid && !lab && pred));
  c.fn += (unsigned)__popcll(__ballot(valid && lab && !pred));
}

__global__ void __launch_bounds__(kMeThreads) margin_eval_kernel(const float* margin, const float* adj,
                                                                 int ngraphs, int n,
                                                                 unsigned long long* hist,
                                                                 unsigned long long* counts) {
  __shared__ unsigned sHist[2 * kEvalBins];
  __shared__ unsigned sRed[kMeThreads / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nn = (long long)n * n;
  const long long c0 = (long long)blockIdx.x * kMeChunk;
  const int len = (int)(nn - c0 < kMeChunk ? nn - c0 : kMeChunk);   // >= 1 by the grid
  const unsigned np1 = (unsigned)n + 1u;

  for (int b = blockIdx.y; b < ngraphs; b += gridDim.y) {
    for (int i = tid; i < 2 * kEvalBins; i += kMeThreads) sHist[i] = 0u;
    __syncthreads();

    const float* m = margin + (long long)b * nn + c0;
    const float* a = adj + (long long)b * nn + c0;
    MeCounts c{0u, 0u, 0u};
    // b N^2 + c0 is misaligned for odd N, and the two bases need not agree
    const bool vec = ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(a)) & 15) == 0;
    const int nv = vec ? len >> 2 : 0;
    if (nv > 0) {
      unsigned r = (unsigned)((unsigned long long)(c0 + 4 * tid) % np1);
      const unsigned step = (4u * kMeThreads) % np1;
      for (int q0 = 0; q0 < nv; q0 += kMeThreads) {
        const int q = q0 + tid;
        const bool in = q < nv;
        f32x4 mv = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
        if (in) {
          mv = *reinterpret_cast<const f32x4*>(m + 4 * q);
          av = *reinterpret_cast<const f32x4*>(a + 4 * q);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) me_count(sHist, mv[k], av[k], in && !me_on_diag(r + k, np1), c);
        r += step;
        if (r >= np1) r -= np1;
      }
    }
    {   // the scalar path: the chunk's tail, or all of a misaligned chunk
      const int s0 = 4 * nv;
      unsigned r = (unsigned)((unsigned long long)(c0 + s0 + tid) % np1);
      const unsigned step = (unsigned)kMeThreads % np1;
      for (int e0 = s0; e0 < len; e0 += kMeThreads) {
        const int e = e0 + tid;
        const bool in = e < len;
        float mv = 0.f, av = 0.f;
        if (in) {
          mv = m[e];
          av = a[e];
        }
        me_count(sHist, mv, av, in && !me_on_diag(r, np1), c);
        r += step;
        if (r >= np1) r -= np1;
      }
    }

    __syncthreads();
    unsigned long long* hg = hist + (long long)b * 2 * kEvalBins;
    for (int i = tid; i < 2 * kEvalBins; i += kMeThreads) {
      const unsigned v = sHist[i];
      if (v) atomicAdd(&hg[i], (unsigned long long)v);
    }
    if (lane == 0) {
      sRed[wave][0] = c.tp;
      sRed[wave][1] = c.fp;
      sRed[wave][2] = c.fn;
    }
    __syncthreads();
    if (tid < 4) {
      unsigned s[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = sRed[0][k] + sRed[1][k] + sRed[2][k] + sRed[3][k];
      // the chunk's other entries, its diagonal pairs among them, are TN
      const unsigned v = tid < 3 ? s[tid] : (unsigned)len - s[0] - s[1] - s[2];
      if (v) atomicAdd(&counts[(long long)b * 4 + tid], (unsigned long long)v);
    }
  }
}

}  // namespace
}  // namespace snd

extern "C" int snd_disent_losses(const double* sse_node, int node_blocks, double node_count,
                                 const double* sse_spatial, int spatial_blocks, double spatial_count,
                                 const double* ce_out, double pair_count, const double* reg_s,
                                 const double* reg_g, const double* reg_sg, double* losses,
                                 snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(sse_node && sse_spatial && ce_out && reg_sg && losses, "snd_disent_losses: null operand");
  SND_CHECK_ARG(node_blocks >= 1 && spatial_blocks >= 1, "snd_disent_losses: block counts %d, %d < 1",
                node_blocks, spatial_blocks);
  SND_CHECK_ARG(node_count > 0.0 && spatial_count > 0.0 && pair_count > 0.0,
                "snd_disent_losses: the counts must be > 0");
  DisentLossArgs a{sse_node, node_blocks, node_count, sse_spatial, spatial_blocks, spatial_count,
                   ce_out, pair_count, reg_s, reg_g, reg_sg, losses};
  hipLaunchKernelGGL(disent_losses_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  SND_LAUNCH_CHECK("disent_losses_kernel");
  return 0;
}

extern "C" size_t snd_margin_eval_workspace(int n_graphs, int n) {
  (void)n_graphs; (void)n;
  return 0;   // every partial sum lives in LDS
}

extern "C" int snd_margin_eval(const float* margin, const float* adj, int n_graphs, int n, long long* hist,
                               long long* counts, int accumulate, void* workspace, size_t workspace_bytes,
                               snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(margin && adj && hist && counts, "snd_margin_eval: null operand");
  SND_CHECK_ARG(n_graphs >= 1 && n >= 1, "snd_margin_eval: empty batch (%d graphs, n=%d)", n_graphs, n);
  const size_t need = snd_margin_eval_workspace(n_graphs, n);
  SND_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace), "snd_margin_eval: workspace %zu < %zu",
                workspace_bytes, need);
  const long long chunks = ((long long)n * n + kMeChunk - 1) / kMeChunk;
  // chunks x 256 threads must stay below 2^32 in the grid's x dimension
  SND_CHECK_ARG(chunks < (1LL << 23), "snd_margin_eval: n=%d too large", n);
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    if (hipMemsetAsync(hist, 0, (size_t)n_graphs * 2 * kEvalBins * 8, s) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)n_graphs * 4 * 8, s) != hipSuccess) {
      set_error("snd_margin_eval: memset failed");
      return SND_ERR_HIP;
    }
  }
  // grid.y is 16-bit: past 65535 graphs a workgroup walks several of them
  const unsigned gy = (unsigned)(n_graphs < 65535 ? n_graphs : 65535);
  hipLaunchKernelGGL(margin_eval_kernel, dim3((unsigned)chunks, gy), dim3(kMeThreads), 0, s, margin, adj,
                     n_graphs, n, reinterpret_cast<unsigned long long*>(hist),
                     reinterpret_cast<unsigned long long*>(counts));
  SND_LAUNCH_CHECK("margin_eval_kernel");
  return 0;
}
