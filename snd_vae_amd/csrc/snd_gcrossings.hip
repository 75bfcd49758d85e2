// Edge crossings of a block-diagonal CSR drawn at its nodes' coordinates (snd_graph_crossings):
// how far a generated spatial network is from planar as embedded.  The graph is snd_graph_motifs'
// mutual-edge graph; the predicate (shared endpoint, fp32 box reject, strict straddle of four
// double orientations with every rounding spelled out) is the definition in include/snd_vae.h.
// Five kernels on one stream.
//
// gx_prep_kernel: a wave per row i.  The first occurrence of each column j (test-and-set in an
// n-bit LDS mask) is looked up in row j (by the lane that holds j when that row has at most 64
// entries, by the whole wave when it is longer); a column found there with j > i is an
// edge (a, b) = (i, j) and is appended to graph g's edge list in the workspace (at rowptr[g n] +
// a cursor taken with one atomic per 64 entries: the order of the list varies between runs, no
// output depends on it), one not found is a one-way arc.  Adds E, sum C(deg, 2), the one-way arcs
// and the zero-length edges, and clears the row's cross_out entries.
//
// gx_plan_kernel: one workgroup.  work[b] = E (E - 1) / 2; a graph above work_cap gets no work
// items; the others T (T + 1) / 2 tile pairs, T = ceil(E / 64); an exclusive prefix over the graphs.
//
// gx_pairs_kernel: the all-pairs test.  A fixed grid of waves; each takes a contiguous range of
// the global item list (one binary search in the prefix, then an incremental walk over (graph,
// e-tile, f-tile >= e-tile)).  A lane holds one e-edge in registers, the wave stages 64 f-edges
// with their boxes in its own LDS, and every lane reads the same four f-boxes per step (broadcast
// reads, in flight together).  The fp32 box test rejects nearly every pair; the survivors test the endpoints
// and then the double predicate.  A crossing raises the lane's own count and an LDS counter of
// the f-edge (32-bit LDS atomic, flushed per tile) and bins its angle in the wave's LDS
// histogram, flushed when the wave leaves a row of tiles.
//
// gx_finish_kernel: per edge the crossing-count and orientation histograms (LDS, flushed with
// 64-bit atomics), the crossed edges, the largest count, cross_out; -1 over a skipped graph's
// cross_out span.  gx_final_kernel: a thread per graph writes counts.
#include "snd_gcrossings.hpp"

namespace snd {

__device__ __forceinline__ void gx_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long gx_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned gx_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ bool gx_skipped(const GraphCrossingsArgs& a, int g) {
  return a.work[g] > (unsigned long long)a.work_cap;
}

// One rounding per operation (__dsub_rn / __dmul_rn / __fsub_rn / ... semantics).  The toolkit's
// versions are plain operators in a header compiled under the default contraction mode, so a
// product and the subtraction that follows it could still be fused after inlining; these are
// compiled with contraction off.
#pragma clang fp contract(off)
__device__ __forceinline__ double gx_dsub(double x, double y) { return x - y; }
__device__ __forceinline__ double gx_dmul(double x, double y) { return x * y; }
__device__ __forceinline__ float gx_fsub(float x, float y) { return x - y; }
__device__ __forceinline__ float gx_fadd(float x, float y) { return x + y; }
__device__ __forceinline__ float gx_fmul(float x, float y) { return x * y; }

// orient(p, q, r) = (qx - px)(ry - py) - (qy - py)(rx - px) in double: seven roundings
__device__ __forceinline__ double gx_orient(float px, float py, float qx, float qy, float rx, float ry) {
  const double t0 = gx_dmul(gx_dsub((double)qx, (double)px), gx_dsub((double)ry, (double)py));
  const double t1 = gx_dmul(gx_dsub((double)qy, (double)py), gx_dsub((double)rx, (double)px));
  return gx_dsub(t0, t1);
}
#pragma clang fp contract(fast)

__device__ __forceinline__ bool gx_opposite(double s, double t) { return (s > 0.0 && t < 0.0) || (s < 0.0 && t > 0.0); }

// e = (a, b) in p = (ax, ay, bx, by), f = (c, d) in q: do they straddle each other strictly?
__device__ __forceinline__ bool gx_straddle(const float4& p, const float4& q) {
  if (!gx_opposite(gx_orient(p.x, p.y, p.z, p.w, q.x, q.y), gx_orient(p.x, p.y, p.z, p.w, q.z, q.w))) return false;
  return gx_opposite(gx_orient(q.x, q.y, q.z, q.w, p.x, p.y), gx_orient(q.x, q.y, q.z, q.w, p.z, p.w));
}

// Condition 2 on boxes with min <= max (or the empty box +inf, -inf): max(exmin, fxmin) <=
// min(exmax, fxmax) is the same as neither exmax < fxmin nor fxmax < exmin, by compares alone.
// Written with max / min so that the four compares are not packed into a vector of booleans.
__device__ __forceinline__ bool gx_overlap(float exmin, float exmax, float eymin, float eymax, const float4& f) {
  return (fmaxf(exmin, f.x) <= fminf(exmax, f.y)) & (fmaxf(eymin, f.z) <= fminf(eymax, f.w));
}

// bin of the acute angle between the two edges, 256 bins over [0, pi / 2]
__device__ __forceinline__ int gx_angle_bin(const float4& p, const float4& q) {
  const float ux = gx_fsub(p.z, p.x), uy = gx_fsub(p.w, p.y), vx = gx_fsub(q.z, q.x), vy = gx_fsub(q.w, q.y);
  const float cr = fabsf(gx_fsub(gx_fmul(ux, vy), gx_fmul(uy, vx)));
  const float dt = fabsf(gx_fadd(gx_fmul(ux, vx), gx_fmul(uy, vy)));
  const float k = floorf(gx_fmul(atan2f(cr, dt), 162.97466f));        // 512 / pi
  return k < 255.f ? (k > 0.f ? (int)k : 0) : 255;                     // a NaN lands in 255
}

// bin of the direction of (ax, ay) -> (bx, by) folded to [0, pi), 256 bins centred on k pi / 256
__device__ __forceinline__ int gx_direction_bin(const float4& p) {
  float ux = gx_fsub(p.z, p.x), uy = gx_fsub(p.w, p.y);
  if (uy < 0.f || (uy == 0.f && ux < 0.f)) {
    ux = -ux;
    uy = -uy;
  }
  const float k = floorf(gx_fadd(gx_fmul(atan2f(uy, ux), 81.48733f), 0.5f));   // 256 / pi
  return (k >= 0.f && k <= 256.f) ? ((int)k & 255) : 0;
}

__global__ void __launch_bounds__(64 * kGxWaves) gx_prep_kernel(GraphCrossingsArgs a) {
  extern __shared__ __attribute__((aligned(8))) unsigned char sRaw[];   // [waves][words] row masks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned* sMask = reinterpret_cast<unsigned*>(sRaw) + wave * a.words;
  const unsigned n = (unsigned)a.n;
  const long long rows = (long long)a.n * a.ngraphs;

  for (int w = lane; w < a.words; w += 64) sMask[w] = 0u;
  gx_wave_sync();

  for (long long i = (long long)blockIdx.x * kGxWaves + wave; i < rows; i += (long long)gridDim.x * kGxWaves) {
    const int g = (int)(i / a.n);
    const unsigned cbase = (unsigned)g * n, li = (unsigned)(i - (long long)cbase);
    const int* rp = a.rowptr + (long long)cbase;
    const int beg = rp[li], end = rp[li + 1];
    if (end <= beg) continue;
    const long long gbase = rp[0];
    unsigned long long* acc = a.acc + (long long)g * kGxAcc;
    const float ax = a.coords[i * a.ldc], ay = a.coords[i * a.ldc + 1];
    unsigned deg = 0, one = 0, zero = 0, up = 0;
    for (int e0 = beg; e0 < end; e0 += 64) {
      const int e = e0 + lane;
      unsigned lc = ~0u;
      if (e < end) {
        lc = (unsigned)a.colidx[e] - cbase;
        if (a.cross_out && e < a.nnz_cap) a.cross_out[e] = 0;
      }
      bool first = false;
      if (lc < n && lc != li) {
        const unsigned bit = 1u << (lc & 31u);
        first = (atomicOr(&sMask[lc >> 5], bit) & bit) == 0u;
      }
      // is i in row j?  A short row j is scanned by the lane that holds it, four loads in flight;
      // a long one by the whole wave
      bool mut = false;
      int lb = 0, le = 0;
      if (first) {
        lb = rp[lc];
        le = rp[lc + 1];
      }
      const bool own = first && le - lb <= kGxOwnScan;
      if (own) {
        for (int ee = lb; ee < le; ee += 4) {
          unsigned v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = ee + u < le ? (unsigned)a.colidx[ee + u] : ~0u;
#pragma unroll
          for (int u = 0; u < 4; ++u) mut |= v[u] == (unsigned)i;
        }
      }
      unsigned long long todo = __ballot(first && !own);
      while (todo) {                           // row j of each first occurrence: is i in it?
        const int k = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const unsigned j = (unsigned)__builtin_amdgcn_readlane((int)lc, k);
        const int jb = rp[j], je = rp[j + 1];
        bool f = false;
        for (int ee = jb + lane; ee < je; ee += 64) f |= (unsigned)a.colidx[ee] == (unsigned)i;
        const bool found = __ballot(f) != 0ull;
        if (lane == k) mut = found;
      }
      const bool edge = first && mut;
      const bool keep = edge && lc > li;
      const unsigned long long m = __ballot(keep);
      const unsigned cnt = (unsigned)__popcll(m);
      if (cnt) {
        unsigned long long cur = 0;
        if (lane == 0) cur = atomicAdd(&acc[GX_E], (unsigned long long)cnt);
        cur = __shfl(cur, 0, 64);
        if (keep) {
          const long long slot = gbase + (long long)cur + gx_prefix(m);
          const long long b = (long long)cbase + lc;
          const float bx = a.coords[b * a.ldc], by = a.coords[b * a.ldc + 1];
          if (slot < a.nnz_cap) {
            a.ept[slot] = make_float4(ax, ay, bx, by);
            a.eab[slot] = li | (lc << 16);
            a.epos[slot] = e;
            a.ecnt[slot] = 0u;
          }
          zero += (ax == bx && ay == by) ? 1u : 0u;
        }
      }
      up += cnt;
      deg += (unsigned)__popcll(__ballot(edge));
      one += (unsigned)__popcll(__ballot(first && !mut));
    }
    gx_wave_sync();
    for (int e = beg + lane; e < end; e += 64) {               // clear what was set
      const unsigned lc = (unsigned)a.colidx[e] - cbase;
      if (lc < n) sMask[lc >> 5] = 0u;
    }
    gx_wave_sync();
    zero = (unsigned)gx_wave_sum(zero);
    if (lane == 0) {
      const unsigned long long d = deg;
      if (d >= 2) atomicAdd(&acc[GX_W], d * (d - 1) / 2);
      if (one) atomicAdd(&acc[GX_ONEWAY], (unsigned long long)one);
      if (zero) atomicAdd(&acc[GX_ZERO], (unsigned long long)zero);
    }
  }
}

__device__ __forceinline__ long long gx_tiles(long long E) { return (E + kGxTile - 1) / kGxTile; }

__global__ void __launch_bounds__(256) gx_plan_kernel(GraphCrossingsArgs a) {
  __shared__ long long sScan[256];
  __shared__ long long sCarry;
  if (threadIdx.x == 0) sCarry = 0;
  __syncthreads();
  for (int g0 = 0; g0 < a.ngraphs; g0 += 256) {
    const int g = g0 + (int)threadIdx.x;
    long long items = 0;
    if (g < a.ngraphs) {
      const long long E = (long long)a.acc[(long long)g * kGxAcc + GX_E];
      const unsigned long long wk = (unsigned long long)E * (unsigned long long)(E > 0 ? E - 1 : 0) / 2ull;
      a.work[g] = wk;
      const long long T = gx_tiles(E);
      if (E >= 2 && wk <= (unsigned long long)a.work_cap) items = T * (T + 1) / 2;
    }
    sScan[threadIdx.x] = items;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const long long v = threadIdx.x >= (unsigned)o ? sScan[threadIdx.x - o] : 0;
      __syncthreads();
      sScan[threadIdx.x] += v;
      __syncthreads();
    }
    const long long carry = sCarry;
    if (g < a.ngraphs) a.item_prefix[g] = carry + sScan[threadIdx.x] - items;
    __syncthreads();
    if (threadIdx.x == 255) sCarry = carry + sScan[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.item_prefix[a.ngraphs] = sCarry;
}

// first item of row et of the upper triangle of T x T tiles
__device__ __forceinline__ long long gx_row_start(long long et, long long T) { return et * T - et * (et - 1) / 2; }

__global__ void __launch_bounds__(64 * kGxWaves) gx_pairs_kernel(GraphCrossingsArgs a) {
  __shared__ float4 sBoxAll[kGxWaves][kGxTile];       // (xmin, xmax, ymin, ymax) of the f-edges
  __shared__ float4 sPtAll[kGxWaves][kGxTile];
  __shared__ unsigned sAbAll[kGxWaves][kGxTile];
  __shared__ unsigned sCntAll[kGxWaves][kGxTile];     // crossings found for the f-edges of this tile
  __shared__ unsigned sHistAll[kGxWaves][kGxBins];    // crossing angles of the current graph
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float4* sBox = sBoxAll[wave];
  float4* sPt = sPtAll[wave];
  unsigned* sAb = sAbAll[wave];
  unsigned* sCnt = sCntAll[wave];
  unsigned* sHist = sHistAll[wave];

  const long long total = a.item_prefix[a.ngraphs];
  const long long nw = (long long)gridDim.x * kGxWaves, w = (long long)blockIdx.x * kGxWaves + wave;
  const long long chunk = (total + nw - 1) / nw;
  long long k = w * chunk;
  const long long k1 = k + chunk < total ? k + chunk : total;
  if (k >= k1) return;

  sCnt[lane] = 0u;
  for (int b = lane; b < kGxBins; b += 64) sHist[b] = 0u;
  gx_wave_sync();

  int g;                                       // the graph of item k: the last one with prefix <= k
  {
    int lo = 0, hi = a.ngraphs - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (a.item_prefix[mid] <= k) lo = mid; else hi = mid - 1;
    }
    g = lo;
  }
  long long E = (long long)a.acc[(long long)g * kGxAcc + GX_E], T = gx_tiles(E);
  long long gbase = a.rowptr[(long long)g * a.n];
  long long et, ft;
  {
    const long long kk = k - a.item_prefix[g];
    const double tt = 2.0 * (double)T + 1.0;
    et = (long long)((tt - sqrt(fmax(tt * tt - 8.0 * (double)kk, 0.0))) * 0.5);
    et = et < 0 ? 0 : (et > T - 1 ? T - 1 : et);
    while (et > 0 && gx_row_start(et, T) > kk) --et;
    while (et < T - 1 && gx_row_start(et + 1, T) <= kk) ++et;
    ft = et + (kk - gx_row_start(et, T));
  }

  long long cur_et = -1, eslot = 0;
  bool valid = false;
  float4 ep = make_float4(0.f, 0.f, 0.f, 0.f);
  float exmin = 0.f, exmax = 0.f, eymin = 0.f, eymax = 0.f;
  unsigned ea = 0, eb = 0, c = 0;
  unsigned long long x = 0;
  unsigned binned = 0u;                        // a bound on what one bin of sHist holds (wave-uniform)

  auto flush_hist = [&]() {
    gx_wave_sync();
    for (int b = lane; b < kGxBins; b += 64) {
      const unsigned v = sHist[b];
      if (v) {
        atomicAdd(reinterpret_cast<unsigned long long*>(a.hist) + ((long long)g * 3 + 2) * kGxBins + b,
                  (unsigned long long)v);
        sHist[b] = 0u;
      }
    }
    gx_wave_sync();
  };
  auto flush_edge = [&]() {                    // the lane's e-edge is done with this row of tiles
    if (valid && c) atomicAdd(&a.ecnt[eslot], c);
    c = 0;
    flush_hist();
    binned = 0u;
    x = gx_wave_sum(x);
    if (lane == 0 && x) atomicAdd(&a.acc[(long long)g * kGxAcc + GX_X], x);
    x = 0;
  };

  for (; k < k1; ++k) {
    if (et != cur_et) {
      const long long idx = et * kGxTile + lane;
      valid = idx < E && gbase + idx < a.nnz_cap;
      eslot = gbase + idx;
      exmin = eymin = INFINITY;                // a lane without an edge: every box is rejected
      exmax = eymax = -INFINITY;
      if (valid) {
        ep = a.ept[eslot];
        const unsigned ab = a.eab[eslot];
        ea = ab & 0xFFFFu;
        eb = ab >> 16;
        exmin = fminf(ep.x, ep.z);
        exmax = fmaxf(ep.x, ep.z);
        eymin = fminf(ep.y, ep.w);
        eymax = fmaxf(ep.y, ep.w);
      }
      cur_et = et;
    }
    const long long f0 = ft * kGxTile;
    const int cntF = (int)(E - f0 < kGxTile ? E - f0 : kGxTile);
    if (lane < cntF && gbase + f0 + lane < a.nnz_cap) {
      const float4 q = a.ept[gbase + f0 + lane];
      sPt[lane] = q;
      sBox[lane] = make_float4(fminf(q.x, q.z), fmaxf(q.x, q.z), fminf(q.y, q.w), fmaxf(q.y, q.w));
      sAb[lane] = a.eab[gbase + f0 + lane];
    } else {
      sBox[lane] = make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);   // past the list: rejected
    }
    gx_wave_sync();
    const bool diag = ft == et;
    // the survivors of the box test: endpoints, then the double predicate
    auto survivor = [&](int j) {
      if (!valid || j >= cntF || (diag && j <= lane)) return;
      const unsigned fab = sAb[j];
      const unsigned fa = fab & 0xFFFFu, fbb = fab >> 16;
      if (ea == fa || ea == fbb || eb == fa || eb == fbb) return;
      const float4 q = sPt[j];
      if (!gx_straddle(ep, q)) return;
      ++c;
      ++x;
      atomicAdd(&sCnt[j], 1u);
      atomicAdd(&sHist[gx_angle_bin(ep, q)], 1u);
    };
    // four f-boxes per step: the four LDS reads are in flight together, and one branch covers them
    for (int j0 = 0; j0 < cntF; j0 += 4) {
      const float4 f0b = sBox[j0], f1b = sBox[j0 + 1], f2b = sBox[j0 + 2], f3b = sBox[j0 + 3];
      if (gx_overlap(exmin, exmax, eymin, eymax, f0b)) survivor(j0);
      if (gx_overlap(exmin, exmax, eymin, eymax, f1b)) survivor(j0 + 1);
      if (gx_overlap(exmin, exmax, eymin, eymax, f2b)) survivor(j0 + 2);
      if (gx_overlap(exmin, exmax, eymin, eymax, f3b)) survivor(j0 + 3);
    }
    gx_wave_sync();
    if (lane < cntF) {
      const unsigned v = sCnt[lane];
      if (v) {
        if (gbase + f0 + lane < a.nnz_cap) atomicAdd(&a.ecnt[gbase + f0 + lane], v);
        sCnt[lane] = 0u;
      }
    }
    gx_wave_sync();
    binned += kGxTile * kGxTile;               // the 32-bit LDS bins are flushed before one can wrap
    if (binned >= 0x80000000u) {
      flush_hist();
      binned = 0u;
    }

    if (++ft == T) {
      flush_edge();
      ++et;
      ft = et;
      if (et == T && k + 1 < k1) {             // the next graph that has items
        do {
          ++g;
        } while (a.item_prefix[g + 1] == a.item_prefix[g]);
        E = (long long)a.acc[(long long)g * kGxAcc + GX_E];
        T = gx_tiles(E);
        gbase = a.rowptr[(long long)g * a.n];
        et = ft = 0;
        cur_et = -1;
      }
    }
  }
  if (cur_et == et) flush_edge();              // the range ended inside a row of tiles
}

__global__ void __launch_bounds__(256) gx_finish_kernel(GraphCrossingsArgs a) {
  __shared__ unsigned sH[2][kGxBins];
  __shared__ unsigned sCrossed, sMax;
  const int g = blockIdx.x / a.bpg, blk = blockIdx.x % a.bpg;
  const long long gbase = a.rowptr[(long long)g * a.n];
  if (gx_skipped(a, g)) {
    if (a.cross_out) {
      const long long gend = a.rowptr[(long long)(g + 1) * a.n];
      for (long long p = gbase + (long long)blk * 256 + threadIdx.x; p < gend && p < a.nnz_cap; p += (long long)a.bpg * 256)
        a.cross_out[p] = -1;
    }
    return;
  }
  for (int b = threadIdx.x; b < 2 * kGxBins; b += 256) (&sH[0][0])[b] = 0u;
  if (threadIdx.x == 0) sCrossed = sMax = 0u;
  __syncthreads();
  const long long E = (long long)a.acc[(long long)g * kGxAcc + GX_E];
  unsigned crossed = 0, mx = 0;
  for (long long i = (long long)blk * 256 + threadIdx.x; i < E && gbase + i < a.nnz_cap; i += (long long)a.bpg * 256) {
    const long long slot = gbase + i;
    const unsigned c = a.ecnt[slot];
    const float4 p = a.ept[slot];
    atomicAdd(&sH[0][c < 255u ? c : 255u], 1u);
    if (!(p.x == p.z && p.y == p.w)) atomicAdd(&sH[1][gx_direction_bin(p)], 1u);
    crossed += c ? 1u : 0u;
    mx = c > mx ? c : mx;
    if (a.cross_out) {
      const int pos = a.epos[slot];
      if (pos >= 0 && pos < a.nnz_cap) a.cross_out[pos] = (int)(c < 0x7FFFFFFFu ? c : 0x7FFFFFFFu);
    }
  }
  if (crossed) atomicAdd(&sCrossed, crossed);
  if (mx) atomicMax(&sMax, mx);
  __syncthreads();
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(a.hist) + (long long)g * 3 * kGxBins;
  for (int b = threadIdx.x; b < 2 * kGxBins; b += 256) {
    const unsigned v = (&sH[0][0])[b];
    if (v) atomicAdd(&hist[b], (unsigned long long)v);
  }
  if (threadIdx.x == 0) {
    unsigned long long* acc = a.acc + (long long)g * kGxAcc;
    if (sCrossed) atomicAdd(&acc[GX_CROSSED], (unsigned long long)sCrossed);
    if (sMax) atomicMax(&acc[GX_MAXC], (unsigned long long)sMax);
  }
}

__global__ void __launch_bounds__(64) gx_final_kernel(GraphCrossingsArgs a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.ngraphs) return;
  long long* out = a.counts + (long long)g * kGxCounts;
  if (gx_skipped(a, g)) {
    for (int k = 0; k < kGxCounts; ++k) out[k] = -1;
    return;
  }
  const unsigned long long* acc = a.acc + (long long)g * kGxAcc;
  out[0] = (long long)acc[GX_E];
  out[1] = (long long)acc[GX_X];
  out[2] = (long long)acc[GX_CROSSED];
  out[3] = (long long)a.work[g] - (long long)acc[GX_W];
  out[4] = (long long)acc[GX_ONEWAY];
  out[5] = (long long)acc[GX_ZERO];
  out[6] = (long long)acc[GX_MAXC];
}

// The most edges a graph of the call can have: half its entries, and no more than C(n, 2).
static long long gx_edge_bound(int n, long long nnz_cap) {
  const long long full = (long long)n * (n - 1) / 2, half = nnz_cap / 2;
  return half < full ? half : full;
}

// Workgroups of the all-pairs kernel: kGxGridPerCu = 8 per compute unit, fewer when the call cannot
// hold that many tile pairs.  The kernel's 96 VGPRs admit five waves per SIMD, so five of the
// eight are resident and the others take the slots of ranges that end early; a grid of five per
// compute unit was measured and is slower (2.56 against 2.46 ms on the bench graphs).
static int graph_crossings_pair_blocks(int ngraphs, int n, long long nnz_cap) {
  const long long T = (gx_edge_bound(n, nnz_cap) + kGxTile - 1) / kGxTile;
  const long long most = (long long)kGxGridPerCu * device_cu_count();
  long long per = T * (T + 1) / 2;
  if (per > most * kGxWaves) per = most * kGxWaves;
  long long items = per * ngraphs;
  long long want = (items + kGxWaves - 1) / kGxWaves;
  if (want > most) want = most;
  return (int)(want < 1 ? 1 : want);
}

static int graph_crossings_finish_bpg(int ngraphs, int n, long long nnz_cap) {
  long long want = (4LL * device_cu_count() + ngraphs - 1) / ngraphs;
  const long long most = (gx_edge_bound(n, nnz_cap) + 255) / 256;
  if (want > most) want = most;
  return (int)(want < 1 ? 1 : want);
}

int launch_graph_crossings(const GraphCrossingsArgs& a, hipStream_t s) {
  const long long fblocks = (long long)a.bpg * a.ngraphs;
  SND_CHECK_ARG(a.bpg >= 1 && fblocks < (1LL << 31), "snd_graph_crossings: %lld workgroups", fblocks);
  if (hipMemsetAsync(a.acc, 0, (size_t)a.ngraphs * kGxAcc * 8, s) != hipSuccess ||
      hipMemsetAsync(a.hist, 0, (size_t)a.ngraphs * 3 * kGxBins * 8, s) != hipSuccess) {
    set_error("snd_graph_crossings: memset failed");
    return SND_ERR_HIP;
  }
  const long long rows = (long long)a.n * a.ngraphs;
  const long long want = (rows + kGxWaves - 1) / kGxWaves, most = 64LL * device_cu_count();
  hipLaunchKernelGGL(gx_prep_kernel, dim3((unsigned)(want < most ? want : most)), dim3(64 * kGxWaves),
                     (size_t)kGxWaves * a.words * 4, s, a);
  SND_LAUNCH_CHECK("gx_prep_kernel");
  hipLaunchKernelGGL(gx_plan_kernel, dim3(1), dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("gx_plan_kernel");
  hipLaunchKernelGGL(gx_pairs_kernel, dim3((unsigned)a.pair_blocks), dim3(64 * kGxWaves), 0, s, a);
  SND_LAUNCH_CHECK("gx_pairs_kernel");
  hipLaunchKernelGGL(gx_finish_kernel, dim3((unsigned)fblocks), dim3(256), 0, s, a);
  SND_LAUNCH_CHECK("gx_finish_kernel");
  hipLaunchKernelGGL(gx_final_kernel, dim3((unsigned)((a.ngraphs + 63) / 64)), dim3(64), 0, s, a);
  SND_LAUNCH_CHECK("gx_final_kernel");
  return 0;
}

static size_t gx_acc_bytes(int n_graphs) { return (size_t)round_up((long long)n_graphs * kGxAcc * 8, 16); }
static size_t gx_prefix_bytes(int n_graphs) { return (size_t)round_up(((long long)n_graphs + 1) * 8, 16); }
static size_t gx_cap(long long nnz_cap) { return (size_t)round_up(nnz_cap > 0 ? nnz_cap : 1, 4); }

}  // namespace snd

extern "C" size_t snd_graph_crossings_workspace(int n_graphs, int n, long long nnz_cap) {
  using namespace snd;
  if (n_graphs < 1 || n < 1 || n > kGxMaxN || (long long)n * n_graphs >= (1LL << 31) || nnz_cap < 0) return 0;
  return gx_acc_bytes(n_graphs) + gx_prefix_bytes(n_graphs) + gx_cap(nnz_cap) * 28;
}

extern "C" int snd_graph_crossings(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                                   const float* coords, int ldc, long long work_cap, long long* counts,
                                   long long* hist, long long* work, int* cross_out, void* workspace,
                                   size_t workspace_bytes, snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(n_graphs >= 1, "snd_graph_crossings: n_graphs=%d < 1", n_graphs);
  SND_CHECK_ARG(n >= 1 && n <= kGxMaxN, "snd_graph_crossings: n=%d not in [1, %d] (local ids are 16-bit on chip)", n,
                kGxMaxN);
  SND_CHECK_ARG((long long)n * n_graphs < (1LL << 31), "snd_graph_crossings: n=%d x %d graphs too large", n, n_graphs);
  SND_CHECK_ARG(nnz_cap >= 0, "snd_graph_crossings: nnz_cap=%lld < 0", nnz_cap);
  SND_CHECK_ARG(work_cap >= 0, "snd_graph_crossings: work_cap=%lld < 0", work_cap);
  SND_CHECK_ARG(ldc >= 2, "snd_graph_crossings: ldc=%d < 2", ldc);
  SND_CHECK_ARG(rowptr && coords && counts && hist && work, "snd_graph_crossings: null operand");
  SND_CHECK_ARG(colidx || nnz_cap == 0, "snd_graph_crossings: colidx is NULL with nnz_cap=%lld", nnz_cap);
  const size_t need = snd_graph_crossings_workspace(n_graphs, n, nnz_cap);
  SND_CHECK_ARG(workspace && workspace_bytes >= need, "snd_graph_crossings: workspace %zu < %zu", workspace_bytes,
                need);
  SND_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "snd_graph_crossings: workspace not 16-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const size_t cap = gx_cap(nnz_cap);
  unsigned char* pre = ws + gx_acc_bytes(n_graphs);
  unsigned char* ept = pre + gx_prefix_bytes(n_graphs);
  GraphCrossingsArgs a{rowptr, colidx, nnz_cap, n, n_graphs, coords, ldc, work_cap, counts, hist,
                       reinterpret_cast<unsigned long long*>(work), cross_out,
                       reinterpret_cast<unsigned long long*>(ws), reinterpret_cast<long long*>(pre),
                       reinterpret_cast<float4*>(ept), reinterpret_cast<unsigned*>(ept + cap * 16),
                       reinterpret_cast<int*>(ept + cap * 20), reinterpret_cast<unsigned*>(ept + cap * 24),
                       (n + 31) / 32, graph_crossings_pair_blocks(n_graphs, n, nnz_cap),
                       graph_crossings_finish_bpg(n_graphs, n, nnz_cap)};
  return launch_graph_crossings(a, (hipStream_t)stream);
}
