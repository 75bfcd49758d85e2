#pragma once
#include "snd_common.hpp"

// The tile body shared by the fp32 zz^T kernels that classify logits on chip
// (zzt_eval_kernel, zzt_edges_kernel): a 128 x 128 tile of L = J J^T per workgroup of four
// waves, J staged 32 k at a time, v_mfma_f32_32x32x2_f32 with k ascending from a zero
// accumulator.  One definition, so the kernels' logits are the same fmaf chain by
// construction (bit for bit the chain of gen_adj_kernel).
namespace snd {

constexpr int kEvT = 128;    // tile rows and columns
constexpr int kEvK = 32;     // k per staged chunk
constexpr int kEvLd = 36;    // floats per staged row: 144-B rows put the 16 lanes of every
                             // ds_read_b128 group on 16 distinct 16-B slots of the bank row

// A staged row holds its 32 k permuted so that one 16-byte read gives a lane the operand
// of four consecutive MFMAs: float 8q + 4h + s is k = 8q + 2s + h (h = lane >> 5 is the
// instruction's k index, s the step), which keeps k ascending across the steps.
// Staging is split into the global loads (into registers, issued one stage ahead so their
// latency passes under the previous chunk's MFMAs) and the LDS stores.  Thread t holds k
// 4j .. 4j + 3 (j = t & 7) of rows (t >> 3) + 32 i, i = 0 .. 3; rows past n and k past d are 0.
__device__ __forceinline__ void eval_load(float4 (&v)[4], const float* Z, int ldz, int d, int n,
                                          int rbase, int k0, bool vec, int tid) {
  const int j = tid & 7, k = k0 + 4 * j;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rbase + (tid >> 3) + 32 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n && k < d) {
      const float* p = Z + (long long)row * ldz + k;
      if (vec && k + 3 < d) {
        v[i] = *reinterpret_cast<const float4*>(p);
      } else {
        v[i].x = p[0];
        if (k + 1 < d) v[i].y = p[1];
        if (k + 2 < d) v[i].z = p[2];
        if (k + 3 < d) v[i].w = p[3];
      }
    }
  }
}

__device__ __forceinline__ void eval_store(float* s, const float4 (&v)[4], int tid) {
  const int j = tid & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float* dst = s + ((tid >> 3) + 32 * i) * kEvLd + (j >> 1) * 8 + (j & 1) * 2;
    *reinterpret_cast<float2*>(dst) = make_float2(v[i].x, v[i].z);
    *reinterpret_cast<float2*>(dst + 4) = make_float2(v[i].y, v[i].w);
  }
}

// The MFMAs of one staged chunk: the wave's 64 x 64 block (rows wr .., columns wc .. of the
// tile) as 2 x 2 accumulators of 32 x 32; rem = d - k0 is the k left from this chunk on.
__device__ __forceinline__ void eval_mfma_chunk(f32x16 (&acc)[2][2], const float* sA, const float* sB,
                                                int rem, int wr, int wc, int l31, int h) {
  // the loop stays rolled: unrolled over a full chunk it takes 256 VGPRs and ran 3 % slower
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

}  // namespace snd
