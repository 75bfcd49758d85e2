// Fused zz^T edge extraction (snd_zzt_edges): the predicted graph of the inner-product
// decoder at a caller-chosen logit threshold, as the block-diagonal CSR, without the logits
// or a dense adjacency reaching HBM.  count -> scan -> fill (snd_edges.hpp); both MFMA
// passes recompute L with the tile body of zzt_eval_kernel (snd_zzt_tile.hpp).
//
// Per tile the epilogue turns the wave's 64 x 64 block into bits: in the C/D layout a lane is
// a column and a register is a row, so one ballot of the predicate per accumulator register
// is the 32-column hit word of two rows.  The words go into a 128 x 128 bit image of the tile
// in LDS (2 KB, plain stores: every (row, word) has one owner).  The count pass popcounts the
// image's rows; the fill pass emits every row's set bits in ascending column order at the
// row's running cursor, so a row's entries leave sorted, tile after tile.
#include "snd_edges.hpp"
#include "snd_eval.hpp"
#include "snd_zzt_tile.hpp"

#include <cmath>

namespace snd {

// The bit image of one wave's block.  C/D element r of a 32 x 32 accumulator is row
// (r & 3) + 8 (r >> 2) + 4 h, column l31: the ballot's low word is row rs, the high word row
// rs + 4.  Lane r keeps register r's ballot and stores its two words after the loop.
// kEdge: the tile holds the diagonal or runs past n, so every pair is checked.
template <bool kEdge>
__device__ __forceinline__ void edges_epilogue(const f32x16 (&acc)[2][2], unsigned* sBits, int n,
                                               int r0, int c0, int wr, int wc, int l31, int h,
                                               float thr, bool incl) {
  const int lane = l31 + 32 * h;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int j = c0 + wc + ni * 32 + l31;
      const int ibase = r0 + wr + mi * 32 + 4 * h;
      unsigned long long mine = 0ull;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rs = (r & 3) + 8 * (r >> 2);
        const float L = acc[mi][ni][r];
        bool p = incl ? L >= thr : L > thr;
        if (kEdge) p = p && j < n && ibase + rs < n && ibase + rs != j;
        const unsigned long long m = __ballot(p);
        if (lane == r) mine = m;
      }
      if (lane < 16) {
        const int row = wr + mi * 32 + (lane & 3) + 8 * (lane >> 2);
        const int w = (wc >> 5) + ni;
        sBits[row * 4 + w] = (unsigned)mine;
        sBits[(row + 4) * 4 + w] = (unsigned)(mine >> 32);
      }
    }
  }
}

// kFill = false: the count pass.  kFill = true: the fill pass.
template <bool kFill>
__global__ void __launch_bounds__(256, 2) zzt_edges_kernel(ZztEdgesArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[kEvT * kEvLd];
  __shared__ __attribute__((aligned(16))) float sB[kEvT * kEvLd];
  __shared__ __attribute__((aligned(16))) unsigned sBits[kEvT * 4];   // [row][column / 32]

  if (kFill) {   // the total does not fit: not one element of colidx is touched
    const long long total = *a.nnz;
    if (total > a.cap || total > 0x7fffffffLL) return;
  }

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
  const int cbase = g * a.n;
  const bool vec = (a.ldz & 3) == 0 && (reinterpret_cast<uintptr_t>(a.z) & 15) == 0;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const float thr = a.threshold;
  const bool incl = a.inclusive != 0;
  int* cell = a.cnt + ((long long)g * a.nsplit + split) * a.n;   // this split's [n] cells

  // count: thread t < 128 sums row r0 + t.  fill: lane r < 32 of wave w holds the cursor of
  // row r0 + 32 w + r (the start of its segment, then advanced tile by tile).
  int mycnt = 0, cur = 0;
  if (kFill) {
    const int row = r0 + 32 * wave + lane;
    if (lane < 32 && row < a.n) cur = cell[row];
  }

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
      __syncthreads();   // the previous chunk's reads and the previous tile's bit image are done
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
      eval_mfma_chunk(acc, sA, sB, a.d - k0, wr, wc, l31, h);
    }

    if (t == strip || r0 + kEvT > a.n || c0 + kEvT > a.n)
      edges_epilogue<true>(acc, sBits, a.n, r0, c0, wr, wc, l31, h, thr, incl);
    else
      edges_epilogue<false>(acc, sBits, a.n, r0, c0, wr, wc, l31, h, thr, incl);
    __syncthreads();     // the bit image is complete

    if (!kFill) {
      if (tid < kEvT) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(&sBits[tid * 4]);
        mycnt += __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
      }
    } else {
      // Wave w emits rows 32 w .. 32 w + 31, a row per step: lane l owns columns l and
      // l + 64, and a hit's position is the cursor plus the set bits below it, so each of
      // the two stores writes one contiguous ascending run.  Rows past n have no bits.
      const unsigned below = (1u << l31) - 1u;
      for (int r = 0; r < 32; ++r) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(&sBits[(32 * wave + r) * 4]);
        const int p0 = __popc(w[0]), p1 = __popc(w[1]), p2 = __popc(w[2]), p3 = __popc(w[3]);
        const int base = __builtin_amdgcn_readlane(cur, r);
        const unsigned wlo = h ? w[1] : w[0], whi = h ? w[3] : w[2];
        const long long lo = base + (h ? p0 : 0) + __popc(wlo & below);
        const long long hi = base + p0 + p1 + (h ? p2 : 0) + __popc(whi & below);
        // lo, hi < total <= cap by construction; the compare keeps any disagreement between
        // the passes (none is possible on one device) inside the buffer
        if (((wlo >> l31) & 1u) && lo < a.cap) a.colidx[lo] = cbase + c0 + lane;
        if (((whi >> l31) & 1u) && hi < a.cap) a.colidx[hi] = cbase + c0 + 64 + lane;
        if (lane == r) cur += p0 + p1 + p2 + p3;
      }
    }
  }

  if (!kFill && tid < kEvT && r0 + tid < a.n) cell[r0 + tid] = mycnt;
}

// One workgroup of 1024 threads scans the B n rows in chunks of 4096, four consecutive rows
// per thread: row totals over the splits, wave scans, the wave totals through LDS, an int64
// carry from chunk to chunk.
constexpr int kScanThreads = 1024, kScanItems = 4;

__global__ void __launch_bounds__(kScanThreads) zzt_edges_scan_kernel(int* cnt, int* rowptr,
                                                                      long long* nnz, int n, int ngraphs,
                                                                      int nsplit) {
  __shared__ long long sWave[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long rows = (long long)n * ngraphs;
  long long carry = 0;
  for (long long base = 0; base < rows; base += kScanThreads * kScanItems) {
    const long long first = base + (long long)kScanItems * tid;
    int tot[kScanItems];
    long long cell0[kScanItems];
    long long sum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      const long long row = first + i;
      tot[i] = 0;
      cell0[i] = 0;
      if (row < rows) {
        const long long g = row / n;
        cell0[i] = g * nsplit * n + (row - g * n);
        for (int s = 0; s < nsplit; ++s) tot[i] += cnt[cell0[i] + (long long)s * n];
      }
      sum += tot[i];
    }
    long long inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const long long v = sWave[w];
      before += w < wave ? v : 0;
      all += v;
    }
    long long off = carry + before + inc - sum;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      const long long row = first + i;
      if (row < rows) {
        rowptr[row] = (int)off;
        long long seg = off;
        for (int s = 0; s < nsplit; ++s) {
          const long long c = cell0[i] + (long long)s * n;
          const int v = cnt[c];
          cnt[c] = (int)seg;
          seg += v;
        }
      }
      off += tot[i];
    }
    carry += all;
    __syncthreads();     // sWave is free for the next chunk
  }
  if (tid == 0) {
    rowptr[rows] = (int)carry;
    *nnz = carry;
  }
}

size_t zzt_edges_workspace(int ngraphs, int n, int nsplit) {
  return (size_t)round_up((long long)ngraphs * n * nsplit * (long long)sizeof(int), 256);
}

int launch_zzt_edges(const ZztEdgesArgs& a, hipStream_t s) {
  SND_CHECK_ARG(a.z && a.rowptr && a.nnz && a.cnt, "zzt_edges: null operand");
  SND_CHECK_ARG(a.n > 0 && a.ngraphs > 0, "zzt_edges: empty batch");
  SND_CHECK_ARG(a.d >= 1 && a.d <= 128, "zzt_edges: d=%d not in [1, 128]", a.d);
  SND_CHECK_ARG(a.ldz >= a.d, "zzt_edges: ldz=%d < d=%d", a.ldz, a.d);
  SND_CHECK_ARG(!std::isnan(a.threshold), "zzt_edges: NaN threshold");
  SND_CHECK_ARG(a.n <= (1 << 24) && (long long)a.n * a.ngraphs < (1LL << 31),
                "zzt_edges: n=%d x %d graphs too large", a.n, a.ngraphs);
  const long long ntiles = (a.n + kEvT - 1) / kEvT;
  SND_CHECK_ARG(a.nsplit >= 1 && a.nsplit <= ntiles, "zzt_edges: bad column split %d", a.nsplit);
  const long long blocks = ntiles * a.nsplit * a.ngraphs;
  SND_CHECK_ARG(blocks < (1LL << 31), "zzt_edges: %lld workgroups", blocks);
  SND_CHECK_ARG(a.colidx == nullptr || a.cap >= 0, "zzt_edges: colidx_cap=%lld < 0", a.cap);
  hipLaunchKernelGGL(zzt_edges_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("zzt_edges_kernel<count>");
  hipLaunchKernelGGL(zzt_edges_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a.cnt, a.rowptr, a.nnz,
                     a.n, a.ngraphs, a.nsplit);
  SND_LAUNCH_CHECK("zzt_edges_scan_kernel");
  if (a.colidx) {
    hipLaunchKernelGGL(zzt_edges_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    SND_LAUNCH_CHECK("zzt_edges_kernel<fill>");
  }
  return 0;
}

}  // namespace snd

static bool edges_shape_ok(int n_graphs, int n, int d) {
  return n > 0 && n_graphs > 0 && d >= 1 && d <= 128 && n <= (1 << 24) &&
         (long long)n * n_graphs < (1LL << 31);
}

extern "C" size_t snd_zzt_edges_workspace(int n_graphs, int n, int d) {
  if (!edges_shape_ok(n_graphs, n, d)) return 0;
  return snd::zzt_edges_workspace(n_graphs, n, snd::zzt_eval_splits(n_graphs, n));
}

extern "C" int snd_zzt_edges(const float* z, int ldz, int n_graphs, int n, int d, float threshold,
                             int inclusive, int* rowptr, int* colidx, long long colidx_cap,
                             long long* nnz_out, void* workspace, size_t workspace_bytes,
                             snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(z && rowptr && nnz_out, "snd_zzt_edges: null operand");
  SND_CHECK_ARG(n > 0 && n_graphs > 0, "snd_zzt_edges: empty batch");
  SND_CHECK_ARG(d >= 1 && d <= 128, "snd_zzt_edges: d=%d not in [1, 128]", d);
  SND_CHECK_ARG(ldz >= d, "snd_zzt_edges: ldz=%d < d=%d", ldz, d);
  SND_CHECK_ARG(!std::isnan(threshold), "snd_zzt_edges: NaN threshold");
  SND_CHECK_ARG(edges_shape_ok(n_graphs, n, d), "snd_zzt_edges: n=%d x %d graphs too large", n, n_graphs);
  const size_t need = snd_zzt_edges_workspace(n_graphs, n, d);
  SND_CHECK_ARG(workspace && workspace_bytes >= need, "snd_zzt_edges: workspace %zu < %zu",
                workspace_bytes, need);
  SND_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "snd_zzt_edges: workspace not 4-byte aligned");
  ZztEdgesArgs a{z, ldz, d, n, n_graphs, threshold, inclusive, rowptr, colidx,
                 colidx ? colidx_cap : 0, nnz_out, static_cast<int*>(workspace),
                 zzt_eval_splits(n_graphs, n)};
  return launch_zzt_edges(a, (hipStream_t)stream);
}
