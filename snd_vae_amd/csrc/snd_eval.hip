// Fused zz^T evaluation (snd_zzt_eval): edge-score histograms and the confusion counts of
// the inner-product decoder without the logits or the predicted adjacency reaching HBM.
//
// One workgroup (4 waves) owns a 128-row strip of one graph and a contiguous range of its
// 128-column tiles.  Per tile: the strip's CSR entries that fall into the tile set bits of
// a 128 x 128 label mask in LDS; J's rows and columns are staged 32 k at a time and each
// wave forms a 64 x 64 block of L with 2 x 2 v_mfma_f32_32x32x2_f32 accumulators (k ascending
// from zero: the fmaf chain of gen_adj_kernel, bit for bit); the epilogue bins every logit
// into the workgroup's LDS histogram.  The flush adds the non-zero bins to the graph's
// int64 histogram with 64-bit vector atomics.
#include "snd_eval.hpp"
#include "snd_zzt_tile.hpp"

namespace snd {

// One increment per lane of the wave.  Logits cluster (an untrained decoder puts every pair
// near 0, a confident one puts most non-edges into the underflow bin), and LDS atomics of one
// instruction to one address serialise, so the wave votes first: when half of it or more
// shares the first lane's cell, those lanes are counted with a ballot and the first lane
// adds the count; the others add their own 1 in the same instruction.  Spread logits fail
// the vote and pay a ballot and some scalar work for it.
__device__ __forceinline__ void eval_count_all(unsigned* sHist, unsigned key, int lane) {
  const unsigned k = __builtin_amdgcn_readfirstlane(key);
  const unsigned c = (unsigned)__popcll(__ballot(key == k));
  const bool merged = c >= 32u;                       // wave-uniform
  if (!merged || key != k || lane == 0) atomicAdd(&sHist[key], (merged && lane == 0) ? c : 1u);
}

// The same for a tile in which some lanes have no pair to count.
__device__ __forceinline__ void eval_count_some(unsigned* sHist, unsigned key, bool pend, int lane) {
  const unsigned long long rem = __ballot(pend);
  if (rem != 0ull) {
    const int leader = __ffsll((long long)rem) - 1;
    const unsigned k = __builtin_amdgcn_readlane(key, leader);
    const bool hit = pend && key == k;
    const unsigned c = (unsigned)__popcll(__ballot(hit));
    if (c >= 32u) {
      if (lane == leader) atomicAdd(&sHist[k], c);
      pend = pend && !hit;
    }
  }
  if (pend) atomicAdd(&sHist[key], 1u);
}

// The epilogue of one wave's 64 x 64 block.  C/D element r of a 32 x 32 accumulator is row
// (r & 3) + 8 (r >> 2) + 4 h, column l31; the lane's labels for its 16 rows of a block are
// bits of one word of the column-major label mask.  kEdge: the tile holds the diagonal or
// runs past n, so every pair is checked; interior tiles skip the checks.  Pairs with
// L == 0 (bin 1024, but not predicted) are rare: a block only notes whether it saw one
// and counts them in a second pass when it did.
template <bool kEdge>
__device__ __forceinline__ void eval_epilogue(const f32x16 (&acc)[2][2], unsigned* sHist,
                                              const unsigned* sMask, int n, int r0, int c0, int wr,
                                              int wc, int l31, int h, unsigned& nz0, unsigned& nz1) {
  const int lane = l31 + 32 * h;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int cl = wc + ni * 32 + l31, j = c0 + cl;
      const unsigned w = sMask[cl * 4 + ((wr + mi * 32) >> 5)] >> (4 * h);
      const int ibase = r0 + wr + mi * 32 + 4 * h;
      bool anyzero = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rs = (r & 3) + 8 * (r >> 2);
        const float L = acc[mi][ni][r];
        const unsigned key = eval_key(L, (w >> rs) & 1u);
        anyzero = anyzero || L == 0.f;
        if (kEdge)
          eval_count_some(sHist, key, j < n && ibase + rs < n && ibase + rs != j, lane);
        else
          eval_count_all(sHist, key, lane);
      }
      if (__ballot(anyzero) != 0ull) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rs = (r & 3) + 8 * (r >> 2);
          const bool valid = !kEdge || (j < n && ibase + rs < n && ibase + rs != j);
          const unsigned zero = (valid && acc[mi][ni][r] == 0.f) ? 1u : 0u;
          const unsigned label = (w >> rs) & 1u;
          nz1 += zero & label;
          nz0 += zero & (label ^ 1u);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256, 2) zzt_eval_kernel(ZztEvalArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[kEvT * kEvLd];
  __shared__ __attribute__((aligned(16))) float sB[kEvT * kEvLd];
  __shared__ unsigned sHist[2 * kEvalBins];
  __shared__ unsigned sMask[kEvT * 4];   // [column][row / 32]: bit row % 32
  __shared__ unsigned sRed[4][4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int ntiles = (a.n + kEvT - 1) / kEvT;
  int bid = blockIdx.x;
  const int strip = bid % ntiles;
  bid /= ntiles;
  const int split = bid % a.nsplit, g = bid / a.nsplit;
  const int t0 = (int)((long long)ntiles * split / a.nsplit);
  const int t1 = (int)((long long)ntiles * (split + 1) / a.nsplit);
  const int r0 = strip * kEvT;
  const float* Z = a.z + (long long)g * a.n * a.ldz;
  const int* rp = a.rowptr + (long long)g * a.n;
  const int cbase = g * a.n;
  const bool vec = (a.ldz & 3) == 0 && (reinterpret_cast<uintptr_t>(a.z) & 15) == 0;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;

  for (int i = tid; i < 2 * kEvalBins; i += 256) sHist[i] = 0u;

  // The strip's CSR entries, 8 lanes per row and 32 rows per pass: the first 32 entries of
  // a row stay in registers as column ids local to the graph (-1: none, or outside it), so
  // the per-tile label scan reads no memory; longer rows scan their remainder from global.
  int ent[4][4], eover[4], eend[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = r0 + (tid >> 3) + 32 * p;
    int beg = 0;
    eend[p] = 0;
    if (row < a.n) {
      beg = rp[row];
      eend[p] = rp[row + 1];
    }
    eover[p] = beg + 32 + (tid & 7);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = beg + 8 * q + (tid & 7);
      int c = -1;
      if (e < eend[p]) c = a.colidx[e] - cbase;
      ent[p][q] = (unsigned)c < (unsigned)a.n ? c : -1;
    }
  }

  unsigned nz0 = 0, nz1 = 0;   // off-diagonal pairs with L == 0, by label
  const int nchunks = (a.d + kEvK - 1) / kEvK;

  float4 ra[4], rb[4];         // the next stage's rows and columns, in flight
  eval_load(ra, Z, a.ldz, a.d, a.n, r0, 0, vec, tid);
  eval_load(rb, Z, a.ldz, a.d, a.n, t0 * kEvT, 0, vec, tid);

  for (int t = t0; t < t1; ++t) {
    const int c0 = t * kEvT;
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    for (int ch = 0; ch < nchunks; ++ch) {
      const int k0 = ch * kEvK;
      __syncthreads();   // the previous chunk's reads and the previous tile's epilogue are done
      if (ch == 0) {
        sMask[tid] = 0u;
        sMask[tid + 256] = 0u;
      }
      eval_store(sA, ra, tid);
      eval_store(sB, rb, tid);
      {                  // loads of the next stage: the next chunk, or the next tile's first
        const bool last = ch + 1 == nchunks;
        const int nt = last ? t + 1 : t, nk = last ? 0 : k0 + kEvK;
        if (nt < t1) {
          eval_load(ra, Z, a.ldz, a.d, a.n, r0, nk, vec, tid);
          eval_load(rb, Z, a.ldz, a.d, a.n, nt * kEvT, nk, vec, tid);
        }
      }
      __syncthreads();
      if (ch == 0) {     // labels of the tile: the rows' CSR entries inside its columns
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int rr = (tid >> 3) + 32 * p;
          const unsigned bit = 1u << (rr & 31);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = ent[p][q] - c0;
            if (ent[p][q] >= 0 && (unsigned)c < (unsigned)kEvT) atomicOr(&sMask[c * 4 + (rr >> 5)], bit);
          }
          for (int e = eover[p]; e < eend[p]; e += 8) {
            const int cg = a.colidx[e] - cbase, c = cg - c0;
            if ((unsigned)cg < (unsigned)a.n && (unsigned)c < (unsigned)kEvT)
              atomicOr(&sMask[c * 4 + (rr >> 5)], bit);
          }
        }
      }
      // eval_mfma_chunk (snd_zzt_tile.hpp) spelled out: calling the helper here moves this
      // kernel's register allocation (251 -> 256 VGPRs), so its loop stays in place
      const int rem = a.d - k0;
      const int nq = rem >= kEvK ? kEvK / 8 : (rem + 7) >> 3;
      for (int q = 0; q < nq; ++q) {
        const int o = q * 8 + h * 4;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(&sA[(wr + l31) * kEvLd + o]);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(&sA[(wr + 32 + l31) * kEvLd + o]);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(&sB[(wc + l31) * kEvLd + o]);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(&sB[(wc + 32 + l31) * kEvLd + o]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b1[s], acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b0[s], acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc[1][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();     // the label mask is complete

    if (t == strip || r0 + kEvT > a.n || c0 + kEvT > a.n)
      eval_epilogue<true>(acc, sHist, sMask, a.n, r0, c0, wr, wc, l31, h, nz0, nz1);
    else
      eval_epilogue<false>(acc, sHist, sMask, a.n, r0, c0, wr, wc, l31, h, nz0, nz1);
  }

  __syncthreads();
  unsigned long long* hg = a.hist + (long long)g * 2 * kEvalBins;
  for (int i = tid; i < 2 * kEvalBins; i += 256) {
    const unsigned v = sHist[i];
    if (v) atomicAdd(&hg[i], (unsigned long long)v);
  }
  // counts from the workgroup's histogram: L > 0 is bin >= 1024 except L == 0 itself.
  // Waves 0-1 sum label 0, waves 2-3 label 1: 16 bins per thread.
  unsigned hi = 0, all = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const unsigned v = sHist[tid * 16 + q];
    all += v;
    hi += (tid & 127) >= 64 ? v : 0u;
  }
  hi = wave_sum_u(hi);
  all = wave_sum_u(all);
  nz0 = wave_sum_u(nz0);
  nz1 = wave_sum_u(nz1);
  if (lane == 0) {
    sRed[wave][0] = hi;
    sRed[wave][1] = all;
    sRed[wave][2] = nz0;
    sRed[wave][3] = nz1;
  }
  __syncthreads();
  if (tid < 4) {
    const unsigned z0 = sRed[0][2] + sRed[1][2] + sRed[2][2] + sRed[3][2];
    const unsigned z1 = sRed[0][3] + sRed[1][3] + sRed[2][3] + sRed[3][3];
    const unsigned fp = sRed[0][0] + sRed[1][0] - z0, neg = sRed[0][1] + sRed[1][1];
    const unsigned tp = sRed[2][0] + sRed[3][0] - z1, pos = sRed[2][1] + sRed[3][1];
    // the strip's diagonal pairs are TN; they lie in the column tile `strip`
    const unsigned diag = (strip >= t0 && strip < t1) ? (unsigned)min(kEvT, a.n - r0) : 0u;
    const unsigned v = tid == 0 ? tp : tid == 1 ? fp : tid == 2 ? pos - tp : neg - fp + diag;
    if (v) atomicAdd(&a.counts[(long long)g * 4 + tid], (unsigned long long)v);
  }
}

// Column splits per strip: enough workgroups for two per compute unit, never more than
// the strip has tiles.  The integer sums make the result independent of the choice.
int zzt_eval_splits(int ngraphs, int n) {
  const long long ntiles = (n + kEvT - 1) / kEvT;
  const long long strips = ntiles * ngraphs;
  long long want = (2LL * device_cu_count() + strips - 1) / strips;
  if (want < 1) want = 1;
  if (want > ntiles) want = ntiles;
  return (int)want;
}

int launch_zzt_eval(const ZztEvalArgs& a, int accumulate, hipStream_t s) {
  SND_CHECK_ARG(a.z && a.rowptr && a.colidx && a.hist && a.counts, "zzt_eval: null operand");
  SND_CHECK_ARG(a.n > 0 && a.ngraphs > 0, "zzt_eval: empty batch");
  SND_CHECK_ARG(a.d >= 1 && a.d <= 128, "zzt_eval: d=%d not in [1, 128]", a.d);
  SND_CHECK_ARG(a.ldz >= a.d, "zzt_eval: ldz=%d < d=%d", a.ldz, a.d);
  // 32-bit workgroup counters (128 n pairs at most) and int row ids
  SND_CHECK_ARG(a.n <= (1 << 24) && (long long)a.n * a.ngraphs < (1LL << 31),
                "zzt_eval: n=%d x %d graphs too large", a.n, a.ngraphs);
  const long long ntiles = (a.n + kEvT - 1) / kEvT;
  SND_CHECK_ARG(a.nsplit >= 1 && a.nsplit <= ntiles, "zzt_eval: bad column split %d", a.nsplit);
  const long long blocks = ntiles * a.nsplit * a.ngraphs;
  SND_CHECK_ARG(blocks < (1LL << 31), "zzt_eval: %lld workgroups", blocks);
  if (!accumulate) {
    if (hipMemsetAsync(a.hist, 0, (size_t)a.ngraphs * 2 * kEvalBins * 8, s) != hipSuccess ||
        hipMemsetAsync(a.counts, 0, (size_t)a.ngraphs * 4 * 8, s) != hipSuccess) {
      set_error("zzt_eval: memset failed");
      return SND_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(zzt_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("zzt_eval_kernel");
  return 0;
}

}  // namespace snd

extern "C" size_t snd_zzt_eval_workspace(int n_graphs, int n, int d) {
  (void)n_graphs; (void)n; (void)d;
  return 0;   // every partial sum lives in LDS
}

extern "C" int snd_zzt_eval(const float* z, int ldz, int n_graphs, int n, int d, const int* rowptr,
                            const int* colidx, long long* hist, long long* counts, int accumulate,
                            void* workspace, size_t workspace_bytes, snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(z && rowptr && colidx && hist && counts, "snd_zzt_eval: null operand");
  SND_CHECK_ARG(n > 0 && n_graphs > 0, "snd_zzt_eval: empty batch");
  SND_CHECK_ARG(d >= 1 && d <= 128, "snd_zzt_eval: d=%d not in [1, 128]", d);
  SND_CHECK_ARG(ldz >= d, "snd_zzt_eval: ldz=%d < d=%d", ldz, d);
  const size_t need = snd_zzt_eval_workspace(n_graphs, n, d);
  SND_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace),
                "snd_zzt_eval: workspace %zu < %zu", workspace_bytes, need);
  ZztEvalArgs a{z, ldz, d, n, n_graphs, rowptr, colidx,
                reinterpret_cast<unsigned long long*>(hist),
                reinterpret_cast<unsigned long long*>(counts), zzt_eval_splits(n_graphs, n)};
  return launch_zzt_eval(a, accumulate, (hipStream_t)stream);
}
