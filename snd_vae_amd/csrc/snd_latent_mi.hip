// Latent-factor mutual information (snd_latent_mi, ABI 25): the matrix every histogram-based
// disentanglement score (MIG, avgMI, modularity) is host arithmetic on, from the encoder
// means z [rows, n_lat] and the generative factors f [rows, n_fac], without either leaving
// the device.  A latency-sized op at the reference's scale (400 latent columns, 3 factors,
// a few thousand graphs: 4 MB read once); the point is exact integer counts and one small
// read-back, not bandwidth.
//
// Four kernels on the stream:
//   range   threads along the columns (row-major z and f are read coalesced), four rows in
//           flight per column, a workgroup per (64 columns, slice of rows); the four row
//           lanes meet in LDS and the slice's lo / hi go to the workspace.
//   final   one thread per column folds the slices: min and max do not depend on order.
//   count   a workgroup per (tile of latent columns x tile of factors, slice of rows) keeps
//           the tile's [cols][facs][nbz][nbf] int32 histogram in LDS (at most 48 KiB).  Rows
//           are taken in chunks of 128: the chunk's factor bins are computed once into LDS
//           and shared by the tile's columns.  Non-zero bins are flushed with 32-bit integer
//           atomics into the cleared joint counts (Guideline 12: the sums that share a
//           destination are made on chip first; integer adds commute, so two runs agree
//           bitwise).
//   mi      one wave per (latent, factor): marginals, the terms in parallel, then lane 0 adds
//           them in index order (a major, b minor), in double.
// No floating-point atomics anywhere.
#include "snd_common.hpp"

#include <cmath>

namespace snd {
namespace {

constexpr int kMiMaxLat = 65536, kMiMaxFac = 64, kMiMaxBins = 32;
constexpr int kMiHistInts = 12288;     // 48 KiB of int32 counters per workgroup
constexpr int kMiTileCols = 8;         // latent columns per workgroup at most
constexpr int kMiChunk = 128;          // rows whose factor bins are staged at a time
constexpr int kMiSliceRows = 256;      // a row slice of the count kernel is at least this long
constexpr int kMiThreads = 256;

// The bin rule of include/snd_vae.h, evaluated in double, left to right.  The clamp is on
// the double, with comparisons a NaN fails: no input can index outside [0, nb).
__device__ __forceinline__ int mi_bin(float v, float lo, float hi, int nb) {
  if (!(hi > lo)) return 0;
  const double t = floor(((double)v - (double)lo) * (double)nb / ((double)hi - (double)lo));
  if (!(t >= 1.0)) return 0;
  return t < (double)nb ? (int)t : nb - 1;
}

struct MiShape {
  const float* z; int ldz;
  const float* f; int ldf;
  int rows, n_lat, n_fac, nbz, nbf;
};

// Column c of the stacked [z | f] matrix.
__device__ __forceinline__ const float* mi_column(const MiShape& s, int c, int& ld) {
  if (c < s.n_lat) {
    ld = s.ldz;
    return s.z + c;
  }
  ld = s.ldf;
  return s.f + (c - s.n_lat);
}

__global__ void __launch_bounds__(kMiThreads) mi_range_kernel(MiShape s, int slice_rows, float* part) {
  __shared__ float sLo[4][64], sHi[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int ncols = s.n_lat + s.n_fac;
  const int col = blockIdx.x * 64 + cx;
  const long long r0 = (long long)blockIdx.y * slice_rows;
  const long long r1 = r0 + slice_rows < s.rows ? r0 + slice_rows : s.rows;
  float lo = INFINITY, hi = -INFINITY;
  if (col < ncols) {
    int ld;
    const float* p = mi_column(s, col, ld);
    for (long long r = r0 + ry; r < r1; r += 4) {
      const float v = p[r * ld];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  sLo[ry][cx] = lo;
  sHi[ry][cx] = hi;
  __syncthreads();
  if (ry == 0 && col < ncols) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      lo = fminf(lo, sLo[k][cx]);
      hi = fmaxf(hi, sHi[k][cx]);
    }
    float* o = part + ((size_t)blockIdx.y * ncols + col) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

__global__ void __launch_bounds__(kMiThreads) mi_range_final_kernel(const float* part, int slices, int ncols,
                                                                   float* rng, float* rng_out) {
  const int col = blockIdx.x * kMiThreads + threadIdx.x;
  if (col >= ncols) return;
  float lo = INFINITY, hi = -INFINITY;
  for (int k = 0; k < slices; ++k) {
    const float* p = part + ((size_t)k * ncols + col) * 2;
    lo = fminf(lo, p[0]);
    hi = fmaxf(hi, p[1]);
  }
  rng[2 * col] = lo;
  rng[2 * col + 1] = hi;
  if (rng_out) {
    rng_out[2 * col] = lo;
    rng_out[2 * col + 1] = hi;
  }
}

struct MiTiles { int tc, tf, ctiles, ftiles, slices, slice_rows; };

// blockIdx.x = column tile * ftiles + factor tile; blockIdx.y = row slice.
// dynamic LDS: [tc * tf * nbz * nbf] counters, then [kMiChunk * tf] factor bins (bytes).
__global__ void __launch_bounds__(kMiThreads) mi_count_kernel(MiShape s, MiTiles t, const float* rng,
                                                             unsigned* joint) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sRaw[];
  const int cell = s.nbz * s.nbf;
  const int hist_ints = t.tc * t.tf * cell;
  unsigned* sH = reinterpret_cast<unsigned*>(sRaw);
  unsigned char* sFb = sRaw + (size_t)hist_ints * 4;
  const int tid = threadIdx.x;
  const int col0 = (int)(blockIdx.x / t.ftiles) * t.tc, k0 = (int)(blockIdx.x % t.ftiles) * t.tf;
  const int tcc = min(t.tc, s.n_lat - col0), tfc = min(t.tf, s.n_fac - k0);   // >= 1 by the grid
  const long long r0 = (long long)blockIdx.y * t.slice_rows;
  const long long r1 = r0 + t.slice_rows < s.rows ? r0 + t.slice_rows : s.rows;

  for (int i = tid; i < hist_ints; i += kMiThreads) sH[i] = 0u;

  for (long long c0 = r0; c0 < r1; c0 += kMiChunk) {
    const int nr = (int)(r1 - c0 < kMiChunk ? r1 - c0 : kMiChunk);
    __syncthreads();                       // the counters are clear; the last chunk's bins were read
    for (int e = tid; e < nr * tfc; e += kMiThreads) {
      const int r = e / tfc, kk = e - r * tfc;
      const float v = s.f[(size_t)(c0 + r) * s.ldf + k0 + kk];
      const float* g = rng + 2 * (s.n_lat + k0 + kk);
      sFb[r * t.tf + kk] = (unsigned char)mi_bin(v, g[0], g[1], s.nbf);
    }
    __syncthreads();
    for (int e = tid; e < nr * tcc; e += kMiThreads) {
      const int r = e / tcc, c = e - r * tcc;
      const float v = s.z[(size_t)(c0 + r) * s.ldz + col0 + c];
      const float* g = rng + 2 * (col0 + c);
      const int a = mi_bin(v, g[0], g[1], s.nbz);
      unsigned* h = sH + (c * t.tf) * cell + a * s.nbf;
      for (int kk = 0; kk < tfc; ++kk) atomicAdd(&h[kk * cell + sFb[r * t.tf + kk]], 1u);
    }
  }
  __syncthreads();

  // joint[l][k][a][b]: the tile's (c, kk) block is contiguous over (a, b) on both sides
  for (int i = tid; i < hist_ints; i += kMiThreads) {
    const unsigned v = sH[i];
    if (v) {
      const int ck = i / cell, ab = i - ck * cell;
      const int c = ck / t.tf, kk = ck - c * t.tf;   // c < tcc and kk < tfc where v != 0
      atomicAdd(&joint[((size_t)(col0 + c) * s.n_fac + (k0 + kk)) * cell + ab], v);
    }
  }
}

// One wave per (l, k).  mi is summed by lane 0 over the terms in index order.
__global__ void __launch_bounds__(64) mi_reduce_kernel(const int* joint, int rows, int n_fac, int nbz, int nbf,
                                                       double* mi, double* hz, double* hf) {
  __shared__ int sC[kMiMaxBins * kMiMaxBins];
  __shared__ int sR[kMiMaxBins], sS[kMiMaxBins];
  __shared__ double sT[kMiMaxBins * kMiMaxBins];
  const int lane = threadIdx.x;
  const int l = (int)(blockIdx.x / (unsigned)n_fac), k = (int)(blockIdx.x % (unsigned)n_fac);
  const int cell = nbz * nbf;
  const int* jc = joint + (size_t)blockIdx.x * cell;
  for (int i = lane; i < cell; i += 64) sC[i] = jc[i];
  __syncthreads();
  if (lane < nbz) {
    int r = 0;
    for (int b = 0; b < nbf; ++b) r += sC[lane * nbf + b];
    sR[lane] = r;
  } else if (lane >= 32 && lane - 32 < nbf) {
    int v = 0;
    for (int a = 0; a < nbz; ++a) v += sC[a * nbf + (lane - 32)];
    sS[lane - 32] = v;
  }
  __syncthreads();
  const double n = (double)rows;
  for (int i = lane; i < cell; i += 64) {
    const int c = sC[i];
    double term = 0.0;
    if (c > 0) {
      const int a = i / nbf, b = i - a * nbf;
      term = ((double)c / n) * log((double)c * n / ((double)sR[a] * (double)sS[b]));
    }
    sT[i] = term;
  }
  __syncthreads();
  if (lane == 0) {
    double acc = 0.0;
    for (int i = 0; i < cell; ++i) acc += sT[i];
    mi[blockIdx.x] = acc;
  } else if (lane == 1 && k == 0) {
    double acc = 0.0;
    for (int a = 0; a < nbz; ++a) {
      const double p = (double)sR[a] / n;
      if (sR[a] > 0) acc += p * log(p);
    }
    hz[l] = -acc;
  } else if (lane == 2 && l == 0) {
    double acc = 0.0;
    for (int b = 0; b < nbf; ++b) {
      const double p = (double)sS[b] / n;
      if (sS[b] > 0) acc += p * log(p);
    }
    hf[k] = -acc;
  }
}

bool mi_shape_ok(int rows, int n_lat, int n_fac, int nbz, int nbf) {
  return rows >= 1 && n_lat >= 1 && n_lat <= kMiMaxLat && n_fac >= 1 && n_fac <= kMiMaxFac && nbz >= 1 &&
         nbz <= kMiMaxBins && nbf >= 1 && nbf <= kMiMaxBins;
}

// Row slices of the range kernel: 256 rows each, at most 1024 of them.
void mi_range_slices(int rows, int& slices, int& slice_rows) {
  slices = cdiv(rows, 256);
  if (slices > 1024) slices = 1024;
  slice_rows = cdiv(rows, slices);
  slices = cdiv(rows, slice_rows);
}

MiTiles mi_tiles(int rows, int n_lat, int n_fac, int nbz, int nbf) {
  const int cell = nbz * nbf;
  MiTiles t;
  t.tf = n_fac < kMiHistInts / cell ? n_fac : kMiHistInts / cell;          // >= 12
  t.tc = kMiHistInts / (t.tf * cell);                                       // >= 1
  if (t.tc > kMiTileCols) t.tc = kMiTileCols;
  if (t.tc > n_lat) t.tc = n_lat;
  t.ctiles = cdiv(n_lat, t.tc);
  t.ftiles = cdiv(n_fac, t.tf);
  // enough workgroups to cover the chip twice, but no slice shorter than kMiSliceRows: every
  // slice clears and flushes a whole histogram
  const long long tiles = (long long)t.ctiles * t.ftiles;
  long long want = (2LL * device_cu_count() + tiles - 1) / tiles;
  const long long most = cdiv(rows, kMiSliceRows);
  if (want > most) want = most;
  if (want > 65535) want = 65535;                                            // grid.y
  if (want < 1) want = 1;
  t.slice_rows = cdiv(rows, want);
  t.slices = cdiv(rows, t.slice_rows);
  return t;
}

struct MiLayout { size_t part, rng, joint, total; };

MiLayout mi_layout(int rows, int n_lat, int n_fac, int nbz, int nbf) {
  int slices, slice_rows;
  mi_range_slices(rows, slices, slice_rows);
  const size_t ncols = (size_t)n_lat + n_fac;
  MiLayout w;
  w.part = 0;
  w.rng = (size_t)round_up((long long)((size_t)slices * ncols * 2 * 4), 16);
  w.joint = w.rng + (size_t)round_up((long long)(ncols * 2 * 4), 16);
  w.total = w.joint + (size_t)n_lat * n_fac * nbz * nbf * 4 + 16;          // + 16: the base is aligned up
  return w;
}

}  // namespace
}  // namespace snd

extern "C" size_t snd_latent_mi_workspace(int rows, int n_lat, int n_fac, int nbz, int nbf) {
  using namespace snd;
  if (!mi_shape_ok(rows, n_lat, n_fac, nbz, nbf)) return 0;
  return mi_layout(rows, n_lat, n_fac, nbz, nbf).total;
}

extern "C" int snd_latent_mi(const float* z, int ldz, const float* f, int ldf, int rows, int n_lat, int n_fac,
                             int nbz, int nbf, double* mi, double* hz, double* hf, float* range, int* joint,
                             void* workspace, size_t workspace_bytes, snd_stream_t stream) {
  using namespace snd;
  SND_CHECK_ARG(z && f && mi && hz && hf, "snd_latent_mi: null operand");
  SND_CHECK_ARG(rows >= 1, "snd_latent_mi: rows=%d < 1", rows);
  SND_CHECK_ARG(n_lat >= 1 && n_lat <= kMiMaxLat, "snd_latent_mi: n_lat=%d not in [1, %d]", n_lat, kMiMaxLat);
  SND_CHECK_ARG(n_fac >= 1 && n_fac <= kMiMaxFac, "snd_latent_mi: n_fac=%d not in [1, %d]", n_fac, kMiMaxFac);
  SND_CHECK_ARG(nbz >= 1 && nbz <= kMiMaxBins && nbf >= 1 && nbf <= kMiMaxBins,
                "snd_latent_mi: bins nbz=%d, nbf=%d not in [1, %d]", nbz, nbf, kMiMaxBins);
  SND_CHECK_ARG(ldz >= n_lat, "snd_latent_mi: ldz=%d < n_lat=%d", ldz, n_lat);
  SND_CHECK_ARG(ldf >= n_fac, "snd_latent_mi: ldf=%d < n_fac=%d", ldf, n_fac);
  const MiLayout w = mi_layout(rows, n_lat, n_fac, nbz, nbf);
  SND_CHECK_ARG(workspace && workspace_bytes >= w.total, "snd_latent_mi: workspace %zu < %zu",
                workspace ? workspace_bytes : (size_t)0, w.total);

  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
  float* part = reinterpret_cast<float*>(base + w.part);
  float* rng = reinterpret_cast<float*>(base + w.rng);
  int* counts = joint ? joint : reinterpret_cast<int*>(base + w.joint);
  const int ncols = n_lat + n_fac, cell = nbz * nbf;
  const MiShape sh{z, ldz, f, ldf, rows, n_lat, n_fac, nbz, nbf};

  if (hipMemsetAsync(counts, 0, (size_t)n_lat * n_fac * cell * 4, s) != hipSuccess) {
    set_error("snd_latent_mi: memset failed");
    return SND_ERR_HIP;
  }
  int slices, slice_rows;
  mi_range_slices(rows, slices, slice_rows);
  hipLaunchKernelGGL(mi_range_kernel, dim3((unsigned)cdiv(ncols, 64), (unsigned)slices), dim3(kMiThreads), 0, s, sh,
                     slice_rows, part);
  SND_LAUNCH_CHECK("mi_range_kernel");
  hipLaunchKernelGGL(mi_range_final_kernel, dim3((unsigned)cdiv(ncols, kMiThreads)), dim3(kMiThreads), 0, s, part,
                     slices, ncols, rng, range);
  SND_LAUNCH_CHECK("mi_range_final_kernel");
  const MiTiles t = mi_tiles(rows, n_lat, n_fac, nbz, nbf);
  const size_t lds = (size_t)t.tc * t.tf * cell * 4 + (size_t)kMiChunk * t.tf;
  hipLaunchKernelGGL(mi_count_kernel, dim3((unsigned)(t.ctiles * t.ftiles), (unsigned)t.slices), dim3(kMiThreads),
                     lds, s, sh, t, rng, reinterpret_cast<unsigned*>(counts));
  SND_LAUNCH_CHECK("mi_count_kernel");
  hipLaunchKernelGGL(mi_reduce_kernel, dim3((unsigned)(n_lat * n_fac)), dim3(64), 0, s, counts, rows, n_fac, nbz, nbf,
                     mi, hz, hf);
  SND_LAUNCH_CHECK("mi_reduce_kernel");
  return 0;
}
