// Forward-only e2e structure decoder (ABI 22): z [B, N, D] -> generated adjacency,
// model.py:193-208 without the CE and the gradients of snd_e2e_head_ce.
//
//   x0 = relu(BN0([z_i | z_j]));  y_l = e2e(x_l) (K = N, TF SAME, pb = (N-1)/2);
//   x_{l+1} = relu(BN_{l+1}(y_l));  logits = relu(BN_adj(y_last)) W + b, the diagonal
//   forced to (1, 0);  margin = l1 - l0;  adj = l1 > l0 (ties 0, tf.argmax).
//
// Layer 0 is factorised.  Its input has pair structure: the left D channels of
// x0[b,i,j,:] depend on i only (a_i = relu(BN0[:D](z_i))), the right D on j only
// (a'_j = relu(BN0[D:](z_j))).  With Wsum_n[c,o] = sum over the taps t that SAME padding
// keeps at position n (0 <= n+t-pb < N) of w[t,c,o]:
//   y0[b,i,j,o] = a_i . Wsum_j[:D,o] + a'_j . Wsum_i[D:,o] + P[b,i,o] + Q[b,j,o] + 2 b[o]
//   P = conv1d_SAME(a, w[:, :D]),  Q = conv1d_SAME(a', w[:, D:])      (per node, K = N)
// so an output costs 2D multiply-adds instead of 2 N 2D and x0 [B, N, N, 2D] is never
// formed.  The kernels:
//   e2e_wsum_kernel   Wsum image [N][2][D4][O4] (zero padded to float4 lanes)
//   e2e_pq_kernel     P, Q [B, N, O0], one workgroup per graph or, for few graphs, per node
//   e2e_l0_kernel     one workgroup per (row i, 4 graphs): the two D-long dot products per
//                     output on (j, 4 o) register tiles; Wsum is read once for the 4 graphs
//   e2e_layer_kernel  a general layer, one workgroup per output row (b, i).  The row and the
//                     column filter share their taps, so their inputs are added first:
//                     out[j,:] = sum_t V_t[j,:] w[t],  V_t[j] = x[b,i,j+t-pb] + x[b,i+t-pb,j]
//                     (N C multiply-adds per output, not 2 N C).  V_t and w[t] are staged
//                     in LDS per tap, the consumer's BN + relu is applied as x is loaded,
//                     outputs sit in (TJ j, 4 o) register tiles.
// The last layer's epilogue (either kernel) applies BN_adj + relu, the 2-column head and
// the argmax; logits never reach HBM.  fp32 FMA throughout, every sum in a fixed order,
// no atomics: two runs are bitwise equal.  Nothing synchronises with or allocates on the
// host, so a call can be captured in a HIP graph.
// The kernels live in snd_e2e_dec.hpp: the training engine (snd_e2e_train.hip) runs the same
// forward.
#include "snd_e2e_dec.hpp"

namespace snd {
namespace {

// yhat = sigmoid(u W + b): the forward half of snd_sigmoid_mse
__global__ void __launch_bounds__(DT) sigmoid_linear_kernel(const float* u, int ldu, long long rows, int cin,
                                                            const float* w, const float* b, int cout, float* y,
                                                            int ldy) {
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= rows * cout) return;
  const int o = (int)(idx % cout);
  const long long r = idx / cout;
  float s = b[o];
  for (int c = 0; c < cin; ++c) s = fmaf(u[r * ldu + c], w[(long long)c * cout + o], s);
  y[r * ldy + o] = 1.f / (1.f + __expf(-s));
}

struct DecLayout {
  size_t act, img, pq, off_a, off_b, off_img, total;
};

// [16-byte slack | act A | max(act B, P Q) | Wsum image]; P and Q are dead once layer 0
// has run, before anything writes act B
inline DecLayout dec_layout(int B, int n, int d, const int* couts, int L) {
  DecLayout s{};
  int widest = 0;
  for (int l = 0; l + 1 < L; ++l) widest = std::max(widest, couts[l]);
  s.act = (size_t)round_up((long long)B * n * n * widest, 4);
  s.img = (size_t)n * 2 * up4(d) * up4(couts[0]);
  s.pq = (size_t)round_up(2LL * B * n * couts[0], 4);
  const size_t second = std::max(L >= 3 ? s.act : (size_t)0, s.pq);
  s.off_a = 0;
  s.off_b = L >= 2 ? s.act : 0;
  s.off_img = s.off_b + second;
  s.total = (s.off_img + s.img) * sizeof(float) + 16;
  return s;
}

}  // namespace
}  // namespace snd

using namespace snd;

static bool dec_shape_ok(int n_graphs, int n, int d, const int* couts, int n_layers) {
  if (n_graphs < 1 || n < 1 || d < 1 || n_layers < 1 || !couts) return false;
  for (int l = 0; l < n_layers; ++l)
    if (couts[l] < 1) return false;
  return true;
}

extern "C" size_t snd_e2e_decode_workspace(int n_graphs, int n, int d, const int* couts, int n_layers) {
  if (!dec_shape_ok(n_graphs, n, d, couts, n_layers)) return 0;
  return dec_layout(n_graphs, n, d, couts, n_layers).total;
}

extern "C" int snd_e2e_decode(const float* z, int ldz, int n_graphs, int n, int d, const snd_e2e_layer_t* layers,
                              int n_layers, const float* head_gamma, const float* head_beta, const float* head_w,
                              const float* head_b, unsigned char* adj, float* margin, void* workspace,
                              size_t workspace_bytes, snd_stream_t stream) {
  SND_CHECK_ARG(n_layers >= 1, "snd_e2e_decode: n_layers %d < 1", n_layers);
  SND_CHECK_ARG(z && layers && head_gamma && head_beta && head_w && head_b && adj && workspace,
                "snd_e2e_decode: null operand");
  SND_CHECK_ARG(n_graphs >= 1 && n >= 1 && d >= 1, "snd_e2e_decode: empty shape (n_graphs %d, n %d, d %d)", n_graphs,
                n, d);
  SND_CHECK_ARG(n_layers <= 16, "snd_e2e_decode: n_layers %d > 16", n_layers);
  int couts[16];
  for (int l = 0; l < n_layers; ++l) {
    SND_CHECK_ARG(layers[l].gamma && layers[l].beta && layers[l].w && layers[l].b,
                  "snd_e2e_decode: null operand in layer %d", l);
    SND_CHECK_ARG(layers[l].cout >= 1, "snd_e2e_decode: layer %d has width %d < 1", l, layers[l].cout);
    SND_CHECK_ARG(layers[l].cout <= kMaxDim, "snd_e2e_decode: layer %d has width %d > %d", l, layers[l].cout, kMaxDim);
    couts[l] = layers[l].cout;
  }
  SND_CHECK_ARG(n <= kMaxDim, "snd_e2e_decode: n %d > %d", n, kMaxDim);
  SND_CHECK_ARG(ldz >= d, "snd_e2e_decode: ldz %d < d %d", ldz, d);
  SND_CHECK_ARG(couts[n_layers - 1] <= kHeadC, "snd_e2e_decode: head channels must be in [1, %d], got %d", kHeadC,
                couts[n_layers - 1]);
  const DecLayout lay = dec_layout(n_graphs, n, d, couts, n_layers);
  SND_CHECK_ARG(workspace_bytes >= lay.total, "snd_e2e_decode: workspace %zu bytes < %zu", workspace_bytes, lay.total);
  SND_CHECK_ARG((long long)n_graphs * n <= 0x7fffffffLL && (n_graphs + DG - 1) / DG <= 65535,
                "snd_e2e_decode: n_graphs %d too large for one call (decode in chunks)", n_graphs);

  hipStream_t st = (hipStream_t)stream;
  float* base = (float*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  float* act[2] = {base + lay.off_a, base + lay.off_b};
  float* P = base + lay.off_b;
  float* Q = P + (size_t)n_graphs * n * couts[0];
  float* img = base + lay.off_img;
  const HeadArgs head{head_gamma, head_beta, head_w, head_b, adj, margin};

  // layer 0, factorised
  const snd_e2e_layer_t& l0 = layers[0];
  const int O0 = couts[0], D4 = up4(d);
  const long long nimg = (long long)n * 2 * D4 * up4(O0);
  hipLaunchKernelGGL(e2e_wsum_kernel, dim3((unsigned)cdiv(nimg, DT)), dim3(DT), 0, st, l0.w, n, d, O0, img);
  SND_LAUNCH_CHECK("e2e_wsum_kernel");
  const int ckpq = chunk_of(D4, 2LL * (n + 1), kLdsFloats - kPqRed);
  const int ng = (int)std::min<long long>(n, std::max<long long>(1, cdiv((long long)n_graphs * n, 1024)));
  hipLaunchKernelGGL(e2e_pq_kernel, dim3((unsigned)n_graphs, (unsigned)cdiv(n, ng)), dim3(DT),
                     sizeof(float) * ((size_t)2 * (n + 1) * ckpq + kPqRed), st, z, ldz, n, d, l0.gamma, l0.beta, l0.w,
                     O0, ckpq, ng, P, Q);
  SND_LAUNCH_CHECK("e2e_pq_kernel");
  L0Args a0{z, ldz, n_graphs, n, d, O0, chunk_of(D4, (long long)DG * (n + 1)), l0.gamma, l0.beta, l0.b,
            img, P, Q, act[0], head};
  const size_t lds0 = sizeof(float) * std::max<size_t>((size_t)DG * (n + 1) * a0.CK, 2 * DT);
  const dim3 grid0((unsigned)n, (unsigned)((n_graphs + DG - 1) / DG));
  if (n_layers == 1) hipLaunchKernelGGL(e2e_l0_kernel<true>, grid0, dim3(DT), lds0, st, a0);
  else hipLaunchKernelGGL(e2e_l0_kernel<false>, grid0, dim3(DT), lds0, st, a0);
  SND_LAUNCH_CHECK("e2e_l0_kernel");

  // general layers: y_{l-1} (act[(l-1) & 1]) -> y_l, the last one straight into the head
  for (int l = 1; l < n_layers; ++l) {
    const snd_e2e_layer_t& L = layers[l];
    const int C = couts[l - 1], O = couts[l];
    LayerArgs a{act[(l - 1) & 1], n, C, O, chunk_of(up4(C), 2LL * n + up4(O) + 2), L.gamma, L.beta, L.w, L.b,
                act[l & 1], head};
    if (l + 1 == n_layers) launch_layer<true>(a, n_graphs, st);
    else launch_layer<false>(a, n_graphs, st);
    SND_LAUNCH_CHECK("e2e_layer_kernel");
  }
  return 0;
}

extern "C" int snd_sigmoid_linear_fwd(const float* u, int ldu, long long rows, int cin, const float* w,
                                      const float* b, int cout, float* yhat, int ldy, snd_stream_t stream) {
  SND_CHECK_ARG(u && w && b && yhat, "snd_sigmoid_linear_fwd: null operand");
  SND_CHECK_ARG(rows >= 1 && cin >= 1 && cout >= 1 && ldu >= cin && ldy >= cout,
                "snd_sigmoid_linear_fwd: bad shape (rows %lld, cin %d, cout %d, ldu %d, ldy %d)", rows, cin, cout, ldu,
                ldy);
  hipLaunchKernelGGL(sigmoid_linear_kernel, dim3((unsigned)cdiv(rows * cout, DT)), dim3(DT), 0, (hipStream_t)stream,
                     u, ldu, rows, cin, w, b, cout, yhat, ldy);
  SND_LAUNCH_CHECK("sigmoid_linear_kernel");
  return 0;
}
