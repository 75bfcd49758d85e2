// Graphlet census of a block-diagonal CSR (snd_graph_motifs): per graph the numbers of induced
// edges, open 2-paths, triangles, 3-edge paths, claws, chordless 4-cycles, tailed triangles,
// diamonds and 4-cliques of the mutual-edge graph G_b ({i, j} an edge iff j in N(i) and i in
// N(j), N as in snd_gstats.hip), from the CSR that DeviceBatch holds or snd_zzt_edges writes.
// Five kernels on one stream; as in graph_stats_kernel a wave owns a row, N(u) is a bit mask in
// LDS, neighbours' rows are read with coalesced loads and totals leave with 64-bit atomics.
//
// gm_work_kernel: a wave per row; with l_i the length of CSR row i, over the entries j of row
// i that count (in block, j != i) a_i = sum l_j and c_i = sum_{j > i} l_j min(l_i, l_j);
// work[b] = sum_i 9 l_i + 4 a_i + c_i bounds the column ids the three kernels below read for
// graph b (gm_mutual: 2 l_i + a_i; gm_wedge: 4 l_i + 2 a_i; gm_clique: 3 l_i + a_i for the rows
// v, and per triangle u < v < w one row w, at most c_u in all).  The kernels below return at
// once for a graph with work[b] > work_cap; gm_final_kernel writes -1 for it.
//
// gm_mutual_kernel: the first occurrence of each column j of row i (test-and-set in the mask)
// is looked up in row j; the columns found are appended to row i of the mutual-edge CSR in the
// workspace (local ids, at rowptr[i]; its length is deg[i]), the others are one-way arcs.  The
// later kernels see a symmetric CSR without duplicates.
//
// gm_wedge_kernel: for row u and every v in N(u) the lanes stride over row v: the entries in
// the mask of N(u) are t(u, v) (ballot / popcount, wave-uniform), and every entry w > u raises
// a 16-bit counter in LDS (two per 32-bit word), which ends as the codegree c(u, w).  A second
// walk over the same rows takes each counter back to zero (atomicAnd returns it once) and adds
// C(c, 2).  Sums: 6T, 2TT', D', sum (d_u - 1)(d_v - 1), 2C4'.
//
// gm_clique_kernel: for an edge u < v the entries w > v of row v inside the mask of N(u) go to
// a list and a second mask; for every listed w the entries x > w of row w inside that mask are
// 4-cliques u < v < w < x, each counted once.  Four rows w are in flight per step.
//
// gm_final_kernel: a thread per graph converts the sums to induced counts.
#include "snd_gmotifs.hpp"

namespace snd {

__device__ __forceinline__ void gm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long wave_sum_ull(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned gm_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Is local id w (any value) a member of the n-bit mask?
__device__ __forceinline__ bool gm_bit(const unsigned* sMask, unsigned w, unsigned n) {
  return w < n && ((sMask[w >> 5] >> (w & 31u)) & 1u);
}

__device__ __forceinline__ bool gm_skipped(const GraphMotifsArgs& a, int g) {
  return a.work[g] > (unsigned long long)a.work_cap;
}

__global__ void __launch_bounds__(256) gm_work_kernel(GraphMotifsArgs a) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)a.n * a.ngraphs;
  const unsigned n = (unsigned)a.n;
  for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (long long)gridDim.x * 4) {
    const long long g = i / a.n;
    const unsigned cbase = (unsigned)(g * a.n), li = (unsigned)(i - g * a.n);
    const int beg = a.rowptr[i], end = a.rowptr[i + 1];
    if (end <= beg) continue;
    const unsigned long long len = (unsigned long long)(end - beg);
    const int* rp = a.rowptr + (long long)cbase;
    unsigned long long s = 0;
    for (int e = beg + lane; e < end; e += 64) {
      const unsigned lc = (unsigned)a.colidx[e] - cbase;
      if (lc < n && lc != li) {
        const int lj = rp[lc + 1] - rp[lc];
        const unsigned long long l = lj > 0 ? (unsigned long long)lj : 0ull;
        s += 4ull * l;
        if (lc > li) s += l * (l < len ? l : len);
      }
    }
    s = wave_sum_ull(s) + 9ull * len;
    if (lane == 0) atomicAdd(&a.work[g], s);
  }
}

__global__ void __launch_bounds__(64 * kGmWaves) gm_mutual_kernel(GraphMotifsArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];   // [waves][words] row masks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  if (gm_skipped(a, g)) return;
  unsigned* sMask = reinterpret_cast<unsigned*>(sRaw) + wave * a.words;
  const unsigned n = (unsigned)a.n;
  const unsigned cbase = (unsigned)g * n;
  const int* rp = a.rowptr + (long long)cbase;

  for (int w = lane; w < a.words; w += 64) sMask[w] = 0u;
  gm_wave_sync();

  unsigned long long tD = 0, tW = 0, tS3 = 0, tOne = 0;       // the wave's totals (wave-uniform)
  for (int li = blk * a.waves + wave; li < a.n; li += a.bpg * a.waves) {
    const int beg = rp[li], end = rp[li + 1];
    const unsigned self = cbase + (unsigned)li;
    unsigned cnt = 0, one = 0;
    for (int e0 = beg; e0 < end; e0 += 64) {
      const int e = e0 + lane;
      unsigned lc = ~0u;
      if (e < end) lc = (unsigned)a.colidx[e] - cbase;
      bool first = false;
      if (lc < n && lc != (unsigned)li) {
        const unsigned bit = 1u << (lc & 31u);
        first = (atomicOr(&sMask[lc >> 5], bit) & bit) == 0u;
      }
      bool mut = false;
      unsigned long long todo = __ballot(first);
      while (todo) {                           // row j of each first occurrence: is i in it?
        const int k = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const unsigned j = (unsigned)__builtin_amdgcn_readlane((int)lc, k);
        const int jb = rp[j], je = rp[j + 1];
        bool f = false;
        for (int ee = jb + lane; ee < je; ee += 64) f |= (unsigned)a.colidx[ee] == self;
        const bool found = __ballot(f) != 0ull;
        if (lane == k) mut = found;
      }
      const bool keep = first && mut;
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const long long pos = (long long)beg + cnt + gm_prefix(m);
        if (pos < a.nnz_cap) a.mcol[pos] = (int)lc;
      }
      cnt += (unsigned)__popcll(m);
      one += (unsigned)__popcll(__ballot(first && !mut));
    }
    gm_wave_sync();
    for (int e = beg + lane; e < end; e += 64) {               // clear what was set
      const unsigned lc = (unsigned)a.colidx[e] - cbase;
      if (lc < n) sMask[lc >> 5] = 0u;
    }
    gm_wave_sync();
    if (lane == 0) a.deg[(long long)cbase + li] = (int)cnt;
    const unsigned long long d = cnt;
    tD += d;
    tOne += one;
    if (d >= 2) tW += d * (d - 1) / 2;
    if (d >= 3) tS3 += d * (d - 1) / 2 * (d - 2) / 3;          // C(d, 2) (d - 2) is divisible by 3
  }
  if (lane == 0) {
    unsigned long long* acc = a.acc + (long long)g * kGmAcc;
    if (tD) atomicAdd(&acc[GM_SUMD], tD);
    if (tW) atomicAdd(&acc[GM_W], tW);
    if (tS3) atomicAdd(&acc[GM_S3P], tS3);
    if (tOne) atomicAdd(&acc[GM_ONEWAY], tOne);
  }
}

__global__ void __launch_bounds__(64 * kGmWaves) gm_wedge_kernel(GraphMotifsArgs a) {
  // per wave: [words] mask of N(u), [(n + 1) / 2] words of two 16-bit codegree counters each
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  if (gm_skipped(a, g)) return;
  const unsigned n = (unsigned)a.n;
  const int halves = (a.n + 1) / 2;
  unsigned* sMask = reinterpret_cast<unsigned*>(sRaw) + wave * (a.words + halves);
  unsigned* sCnt = sMask + a.words;
  const unsigned cbase = (unsigned)g * n;
  const int* rp = a.rowptr + (long long)cbase;
  const int* dg = a.deg + (long long)cbase;

  for (int w = lane; w < a.words + halves; w += 64) sMask[w] = 0u;
  gm_wave_sync();

  unsigned long long tT6 = 0, tTT2 = 0, tDp = 0, tP = 0;       // wave-uniform
  unsigned long long c2 = 0;                                   // per lane
  for (int li = blk * a.waves + wave; li < a.n; li += a.bpg * a.waves) {
    const unsigned u = (unsigned)li;
    const int beg = rp[li], du = dg[li];
    if (du < 1) continue;
    for (int e = lane; e < du; e += 64) {
      const unsigned v = (unsigned)a.mcol[beg + e];
      if (v < n) atomicOr(&sMask[v >> 5], 1u << (v & 31u));
    }
    gm_wave_sync();

    unsigned long long sumT = 0;
    for (int pass = 0; pass < 2; ++pass) {     // 0: t(u, v) and the counters; 1: the counters back to zero
      for (int e0 = 0; e0 < du; e0 += 64) {
        unsigned vl = ~0u;
        int vb = 0, vd = 0;
        if (e0 + lane < du) vl = (unsigned)a.mcol[beg + e0 + lane];
        if (vl < n) {
          vb = rp[vl];
          vd = dg[vl];
        }
        const int cnt = min(64, du - e0);
        for (int k = 0; k < cnt; ++k) {
          const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)vl, k);
          const int b0 = __builtin_amdgcn_readlane(vb, k), dv = __builtin_amdgcn_readlane(vd, k);
          unsigned t = 0;
          for (int s0 = 0; s0 < dv; s0 += 64) {
            unsigned w = ~0u;
            if (s0 + lane < dv) w = (unsigned)a.mcol[b0 + s0 + lane];
            const bool up = w < n && w > u;
            const unsigned sh = (w & 1u) * 16u;
            if (pass == 0) {
              t += (unsigned)__popcll(__ballot(gm_bit(sMask, w, n)));
              if (up) atomicAdd(&sCnt[w >> 1], 1u << sh);
            } else if (up) {
              const unsigned long long c = (atomicAnd(&sCnt[w >> 1], ~(0xFFFFu << sh)) >> sh) & 0xFFFFu;
              c2 += c * (c - (c ? 1ull : 0ull)) / 2;
            }
          }
          if (pass == 0) {
            sumT += t;
            if (v < n && v > u) {
              tDp += (unsigned long long)t * (t ? t - 1u : 0u) / 2;
              tP += (unsigned long long)(du - 1) * (unsigned long long)(dv > 0 ? dv - 1 : 0);
            }
          }
        }
      }
      gm_wave_sync();
    }
    tT6 += sumT;
    if (du >= 2) tTT2 += sumT * (unsigned long long)(du - 2);

    for (int e = lane; e < du; e += 64) {
      const unsigned v = (unsigned)a.mcol[beg + e];
      if (v < n) sMask[v >> 5] = 0u;
    }
    gm_wave_sync();
  }
  c2 = wave_sum_ull(c2);
  if (lane == 0) {
    unsigned long long* acc = a.acc + (long long)g * kGmAcc;
    if (tT6) atomicAdd(&acc[GM_T6], tT6);
    if (tTT2) atomicAdd(&acc[GM_TT2], tTT2);
    if (tDp) atomicAdd(&acc[GM_DP], tDp);
    if (tP) atomicAdd(&acc[GM_PSUM], tP);
    if (c2) atomicAdd(&acc[GM_C4P2], c2);
  }
}

__global__ void __launch_bounds__(64 * kGmWaves) gm_clique_kernel(GraphMotifsArgs a) {
  // per wave: [words] mask of N(u), [words] mask of the listed common neighbours, [n] 16-bit list
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  if (gm_skipped(a, g)) return;
  const unsigned n = (unsigned)a.n;
  const int halves = (a.n + 1) / 2;
  unsigned* sMask = reinterpret_cast<unsigned*>(sRaw) + wave * (2 * a.words + halves);
  unsigned* sMask2 = sMask + a.words;
  unsigned short* sList = reinterpret_cast<unsigned short*>(sMask2 + a.words);
  const unsigned cbase = (unsigned)g * n;
  const int* rp = a.rowptr + (long long)cbase;
  const int* dg = a.deg + (long long)cbase;

  for (int w = lane; w < 2 * a.words; w += 64) sMask[w] = 0u;
  gm_wave_sync();

  unsigned long long k4 = 0;                                   // per lane
  for (int li = blk * a.waves + wave; li < a.n; li += a.bpg * a.waves) {
    const unsigned u = (unsigned)li;
    const int beg = rp[li], du = dg[li];
    if (du < 3) continue;                                      // a 4-clique's nodes have degree >= 3
    for (int e = lane; e < du; e += 64) {
      const unsigned v = (unsigned)a.mcol[beg + e];
      if (v < n) atomicOr(&sMask[v >> 5], 1u << (v & 31u));
    }
    gm_wave_sync();

    for (int e0 = 0; e0 < du; e0 += 64) {
      unsigned vl = ~0u;
      int vb = 0, vd = 0;
      if (e0 + lane < du) vl = (unsigned)a.mcol[beg + e0 + lane];
      if (vl < n) {
        vb = rp[vl];
        vd = dg[vl];
      }
      const int cnt = min(64, du - e0);
      for (int k = 0; k < cnt; ++k) {
        const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)vl, k);
        const int b0 = __builtin_amdgcn_readlane(vb, k), dv = __builtin_amdgcn_readlane(vd, k);
        if (!(v < n && v > u) || dv < 3) continue;

        int len = 0;                           // the common neighbours w > v of u and v
        for (int s0 = 0; s0 < dv; s0 += 64) {
          unsigned w = ~0u;
          if (s0 + lane < dv) w = (unsigned)a.mcol[b0 + s0 + lane];
          const bool hit = w > v && gm_bit(sMask, w, n);
          const unsigned long long m = __ballot(hit);
          if (hit) {
            const int pos = len + (int)gm_prefix(m);
            if (pos < a.n) sList[pos] = (unsigned short)w;
            atomicOr(&sMask2[w >> 5], 1u << (w & 31u));
          }
          len += __popcll(m);
        }
        len = min(len, a.n);
        gm_wave_sync();

        if (len >= 2) {
          for (int q = 0; q < len; q += 4) {   // four rows w in flight; slots past len hold an empty row
            unsigned ww[4], xx[4];
            int w0[4], w1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              ww[r] = 0u;
              w0[r] = w1[r] = 0;
              if (q + r < len) {
                ww[r] = (unsigned)__builtin_amdgcn_readfirstlane((int)sList[q + r]);
                w0[r] = rp[ww[r]];
                w1[r] = w0[r] + dg[ww[r]];
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              xx[r] = ~0u;
              if (w0[r] + lane < w1[r]) xx[r] = (unsigned)a.mcol[w0[r] + lane];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) k4 += (xx[r] > ww[r] && gm_bit(sMask2, xx[r], n)) ? 1ull : 0ull;
#pragma unroll
            for (int r = 0; r < 4; ++r) {      // rows w longer than one wave load
              for (int ee = w0[r] + 64 + lane; ee < w1[r]; ee += 64) {
                const unsigned x = (unsigned)a.mcol[ee];
                k4 += (x > ww[r] && gm_bit(sMask2, x, n)) ? 1ull : 0ull;
              }
            }
          }
        }
        gm_wave_sync();
        for (int q = lane; q < len; q += 64) sMask2[sList[q] >> 5] = 0u;
        gm_wave_sync();
      }
    }

    for (int e = lane; e < du; e += 64) {
      const unsigned v = (unsigned)a.mcol[beg + e];
      if (v < n) sMask[v >> 5] = 0u;
    }
    gm_wave_sync();
  }
  k4 = wave_sum_ull(k4);
  if (lane == 0 && k4) atomicAdd(&a.acc[(long long)g * kGmAcc + GM_K4], k4);
}

__global__ void __launch_bounds__(64) gm_final_kernel(GraphMotifsArgs a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.ngraphs) return;
  long long* out = a.census + (long long)g * kGmCensus;
  if (gm_skipped(a, g)) {
    for (int k = 0; k < kGmCensus; ++k) out[k] = -1;
    return;
  }
  const unsigned long long* acc = a.acc + (long long)g * kGmAcc;
  const long long E = (long long)(acc[GM_SUMD] / 2), W = (long long)acc[GM_W], S3p = (long long)acc[GM_S3P];
  const long long T = (long long)(acc[GM_T6] / 6), TTp = (long long)(acc[GM_TT2] / 2);
  const long long Dp = (long long)acc[GM_DP], P3p = (long long)acc[GM_PSUM] - 3 * T;
  const long long C4p = (long long)(acc[GM_C4P2] / 2), K4 = (long long)acc[GM_K4];
  const long long D = Dp - 6 * K4;
  const long long C4 = C4p - D - 3 * K4;
  const long long TT = TTp - 4 * D - 12 * K4;
  const long long S3 = S3p - TT - 2 * D - 4 * K4;
  const long long P3 = P3p - 2 * TT - 4 * C4 - 6 * D - 12 * K4;
  out[0] = E;
  out[1] = W - 3 * T;
  out[2] = T;
  out[3] = P3;
  out[4] = S3;
  out[5] = C4;
  out[6] = TT;
  out[7] = D;
  out[8] = K4;
  out[9] = (long long)acc[GM_ONEWAY];
}

// Workgroups per graph of the counting kernels: eight four-wave or four one-wave workgroups
// per compute unit over the batch (the LDS of the large layout admits four), never more than
// the graph has groups of rows.  Integer sums: the result does not depend on the choice.
static int graph_motifs_blocks_per_graph(int ngraphs, int n, int waves) {
  const long long groups = ((long long)n + waves - 1) / waves;
  long long want = ((waves > 1 ? 8LL : 4LL) * device_cu_count() + ngraphs - 1) / ngraphs;
  if (want < 1) want = 1;
  if (want > groups) want = groups;
  return (int)want;
}

int launch_graph_motifs(const GraphMotifsArgs& a, hipStream_t s) {
  const long long blocks = (long long)a.bpg * a.ngraphs;
  SND_CHECK_ARG(a.bpg >= 1 && blocks < (1LL << 31), "snd_graph_motifs: %lld workgroups", blocks);
  if (hipMemsetAsync(a.work, 0, (size_t)a.ngraphs * 8, s) != hipSuccess ||
      hipMemsetAsync(a.acc, 0, (size_t)a.ngraphs * kGmAcc * 8, s) != hipSuccess) {
    set_error("snd_graph_motifs: memset failed");
    return SND_ERR_HIP;
  }
  const long long rows = (long long)a.n * a.ngraphs;
  const long long want = (rows + 3) / 4, most = 64LL * device_cu_count();
  hipLaunchKernelGGL(gm_work_kernel, dim3((unsigned)(want < most ? want : most)), dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("gm_work_kernel");
  const dim3 grid((unsigned)blocks), block(64 * a.waves);
  const size_t halves = ((size_t)a.n + 1) / 2;
  hipLaunchKernelGGL(gm_mutual_kernel, grid, block, (size_t)a.waves * a.words * 4, s, a);
  SND_LAUNCH_CHECK("gm_mutual_kernel");
  hipLaunchKernelGGL(gm_wedge_kernel, grid, block, (size_t)a.waves * (a.words + halves) * 4, s, a);
  SND_LAUNCH_CHECK("gm_wedge_kernel");
  hipLaunchKernelGGL(gm_clique_kernel, grid, block, (size_t)a.waves * graph_motifs_wave_lds(a.n), s, a);
  SND_LAUNCH_CHECK("gm_clique_kernel");
  hipLaunchKernelGGL(gm_final_kernel, dim3((unsigned)((a.ngraphs + 63) / 64)), dim3(64), 0, s, a);
  SND_LAUNCH_CHECK("gm_final_kernel");
  return 0;
}

static size_t gm_acc_bytes(int n_graphs) { return (size_t)round_up((long long)n_graphs * kGmAcc * 8, 16); }
static size_t gm_deg_bytes(int n_graphs, int n) { return (size_t)round_up((long long)n_graphs * n * 4, 16); }

}  // namespace snd

extern "C" size_t snd_graph_motifs_workspace(int n_graphs, int n, long long nnz_cap) {
  using namespace snd;
  if (n_graphs < 1 || n < 1 || n > kGmMaxN || (long long)n * n_graphs >= (1LL << 31) || nnz_cap < 0) return 0;
  return gm_acc_bytes(n_graphs) + gm_deg_bytes(n_graphs, n) + (size_t)round_up((nnz_cap > 0 ? nnz_cap : 1) * 4, 16);
}

extern "C" int snd_graph_motifs(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                                long long work_cap, long long* census, long long* work, void* workspace,
                                size_t workspace_bytes, snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(n_graphs >= 1, "snd_graph_motifs: n_graphs=%d < 1", n_graphs);
  SND_CHECK_ARG(n >= 1 && n <= kGmMaxN, "snd_graph_motifs: n=%d not in [1, %d] (local ids are 16-bit on chip)", n,
                kGmMaxN);
  SND_CHECK_ARG((long long)n * n_graphs < (1LL << 31), "snd_graph_motifs: n=%d x %d graphs too large", n, n_graphs);
  SND_CHECK_ARG(nnz_cap >= 0, "snd_graph_motifs: nnz_cap=%lld < 0", nnz_cap);
  SND_CHECK_ARG(work_cap >= 0, "snd_graph_motifs: work_cap=%lld < 0", work_cap);
  SND_CHECK_ARG(rowptr && census && work, "snd_graph_motifs: null operand");
  SND_CHECK_ARG(colidx || nnz_cap == 0, "snd_graph_motifs: colidx is NULL with nnz_cap=%lld", nnz_cap);
  const size_t need = snd_graph_motifs_workspace(n_graphs, n, nnz_cap);
  SND_CHECK_ARG(workspace && workspace_bytes >= need, "snd_graph_motifs: workspace %zu < %zu", workspace_bytes, need);
  SND_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "snd_graph_motifs: workspace not 8-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const int waves = graph_motifs_waves(n);
  GraphMotifsArgs a{rowptr, colidx, nnz_cap, n, n_graphs, work_cap, census,
                    reinterpret_cast<unsigned long long*>(work),
                    reinterpret_cast<unsigned long long*>(ws),
                    reinterpret_cast<int*>(ws + gm_acc_bytes(n_graphs)),
                    reinterpret_cast<int*>(ws + gm_acc_bytes(n_graphs) + gm_deg_bytes(n_graphs, n)),
                    (n + 31) / 32, waves, graph_motifs_blocks_per_graph(n_graphs, n, waves)};
  return launch_graph_motifs(a, (hipStream_t)stream);
}
