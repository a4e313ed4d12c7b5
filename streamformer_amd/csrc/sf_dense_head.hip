// Dense feature projection of the segmentation head (reference modeling:1786-1795): on ALL token rows
//   a = x Wv^T + bv ;  y = a Wo^T + bo ;  out = y + fc2(gelu(fc1(LayerNorm(y))))
// with the head's own copies of the pooling head's value projection, out_proj, layernorm and mlp (modeling:1764-1779).
// Four Linears, one LayerNorm, one GELU at M = B T N rows: the work of an encoder MLP block, so forward and backward run on
// the training step's launchers (sf_launch_gemm in the training arithmetic: bf16 operands, fp32 accumulation; sf_launch_wgrad
// with its riding bias gradient; the LayerNorm / GELU backward kernels of sf_train_kernels.hip).  No GEMM kernel of its own: the one
// kernel here casts the fp32 parameters to bf16 working copies (row-major and transposed, intermediate width zero-padded to 64).
// The caller owns the workspace; it carries the forward's saved tensors to the backward.
#include "sf_common.h"
#include "sf_internal.h"
#include "sf_train.h"
#include <string.h>

// parameter order of both pointer tables
enum { DH_WV_W = 0, DH_WV_B, DH_VP_W, DH_VP_B, DH_LN_G, DH_LN_B, DH_FC1_W, DH_FC1_B, DH_FC2_W, DH_FC2_B, DH_NPARAM };

// w fp32 [N, K] -> wb bf16 [Np, Kp] and wT bf16 [Kp, Np], zero past N / K
__global__ __launch_bounds__(256) void sf_dh_prep_kernel(const float* __restrict__ w, int N, int K, int Np, int Kp, bf16_t* __restrict__ wb,
                                                         bf16_t* __restrict__ wT) {
  __shared__ float tile[32][33];
  const int n0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, k = k0 + tx;
    const float v = (n < N && k < K) ? w[(size_t)n * K + k] : 0.f;
    tile[r][tx] = v;
    if (n < Np && k < Kp) wb[(size_t)n * Kp + k] = (bf16_t)f2bf(v);
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    if (n < Np && k < Kp) wT[(size_t)k * Np + n] = (bf16_t)f2bf(tile[tx][r]);
  }
}

struct DhWs {
  bf16_t *wv, *wvT, *vp, *vpT, *fc1, *fc1T, *fc2, *fc2T;
  float* b1;                                   // fc1 bias, padded
  bf16_t *xb, *a, *ln, *pre, *act;             // saved by the forward
  float* y;                                    // pre-LayerNorm rows
  bf16_t *g_bf, *d_wide, *d_a;                 // backward scratch
  float *d_ln, *d_y;
  float *wg_partial, *cs_partial, *ln_partial;
  size_t bytes;
};
static DhWs dh_carve(void* base, size_t M, size_t D, size_t I) {
  const size_t Ip = (I + 63) / 64 * 64;
  DhWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = (char*)base + off; off += (bytes + 255) & ~(size_t)255; return (void*)p; };
  w.wv = (bf16_t*)take(D * D * 2); w.wvT = (bf16_t*)take(D * D * 2);
  w.vp = (bf16_t*)take(D * D * 2); w.vpT = (bf16_t*)take(D * D * 2);
  w.fc1 = (bf16_t*)take(Ip * D * 2); w.fc1T = (bf16_t*)take(Ip * D * 2);
  w.fc2 = (bf16_t*)take(Ip * D * 2); w.fc2T = (bf16_t*)take(Ip * D * 2);
  w.b1 = (float*)take(Ip * 4);
  w.xb = (bf16_t*)take(M * D * 2); w.a = (bf16_t*)take(M * D * 2); w.ln = (bf16_t*)take(M * D * 2);
  w.pre = (bf16_t*)take(M * Ip * 2); w.act = (bf16_t*)take(M * Ip * 2);
  w.y = (float*)take(M * D * 4);
  w.g_bf = (bf16_t*)take(M * D * 2); w.d_wide = (bf16_t*)take(M * Ip * 2); w.d_a = (bf16_t*)take(M * D * 2);
  w.d_ln = (float*)take(M * D * 4); w.d_y = (float*)take(M * D * 4);
  size_t wp = sf_wgrad_partial_floats((int)M, (int)D, (int)I);
  const size_t c2 = sf_wgrad_partial_floats((int)M, (int)I, (int)D), c3 = sf_wgrad_partial_floats((int)M, (int)D, (int)D);
  if (c2 > wp) wp = c2;
  if (c3 > wp) wp = c3;
  w.wg_partial = (float*)take(wp * 4);
  w.cs_partial = (float*)take(sf_colsum_partial_floats((int)(Ip > D ? Ip : D)) * 4);
  w.ln_partial = (float*)take(sf_ln_bwd_partial_floats((int)D) * 4);
  w.bytes = off;
  return w;
}

static int dh_check(const char* who, int M, int D, int I) {
  if (M <= 0 || D <= 0 || I <= 0) return sf_set_err(SF_ERR_INVALID, "%s: bad shape M=%d D=%d I=%d", who, M, D, I);
  if (D % 64) return sf_set_err(SF_ERR_INVALID, "%s: hidden_size %d must be a multiple of 64", who, D);
  const size_t Ip = ((size_t)I + 63) / 64 * 64;
  if ((size_t)M * (Ip > (size_t)D ? Ip : (size_t)D) * 2 >= ((size_t)1 << 32))
    return sf_set_err(SF_ERR_CAPACITY, "%s: %d rows x %zu columns exceed the 32-bit buffer offsets of the GEMM kernels", who, M, Ip);
  return SF_OK;
}

extern "C" size_t sf_dense_head_workspace_bytes(int M, int D, int I) {
  if (M <= 0 || D <= 0 || I <= 0) return 0;
  return dh_carve(nullptr, (size_t)M, (size_t)D, (size_t)I).bytes;
}

extern "C" int sf_dense_head_forward(const float* x, int M, int D, int I, float eps, const float* const* params, float* out, void* workspace,
                                     size_t workspace_bytes, sf_stream stream) {
  int rc = dh_check("sf_dense_head_forward", M, D, I);
  if (rc) return rc;
  if (!x || !params || !out || !workspace) return sf_set_err(SF_ERR_INVALID, "sf_dense_head_forward: null buffer");
  for (int i = 0; i < DH_NPARAM; ++i)
    if (!params[i]) return sf_set_err(SF_ERR_INVALID, "sf_dense_head_forward: parameter %d is null", i);
  const DhWs w = dh_carve(workspace, M, D, I);
  if (workspace_bytes < w.bytes) return sf_set_err(SF_ERR_WORKSPACE, "sf_dense_head_forward: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const int Ip = (I + 63) / 64 * 64;
  // fp32 parameters -> bf16 working copies (every call: the parameters train)
  HIP_TRY(sf_launch(sf_dh_prep_kernel, dim3(D / 32, D / 32), dim3(256), 0, s, params[DH_WV_W], D, D, D, D, w.wv, w.wvT));
  HIP_TRY(sf_launch(sf_dh_prep_kernel, dim3(D / 32, D / 32), dim3(256), 0, s, params[DH_VP_W], D, D, D, D, w.vp, w.vpT));
  HIP_TRY(sf_launch(sf_dh_prep_kernel, dim3(D / 32, Ip / 32), dim3(256), 0, s, params[DH_FC1_W], I, D, Ip, D, w.fc1, w.fc1T));
  HIP_TRY(sf_launch(sf_dh_prep_kernel, dim3(Ip / 32, D / 32), dim3(256), 0, s, params[DH_FC2_W], D, I, D, Ip, w.fc2, w.fc2T));
  const float* b1 = params[DH_FC1_B];
  if (Ip != I) {
    HIP_TRY(hipMemsetAsync(w.b1, 0, (size_t)Ip * 4, s));
    HIP_TRY(hipMemcpyAsync(w.b1, params[DH_FC1_B], (size_t)I * 4, hipMemcpyDeviceToDevice, s));
    b1 = w.b1;
  }
  HIP_TRY(sf_launch_split(x, w.xb, nullptr, (size_t)M * D, s));
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.xb, w.wv, params[DH_WV_B], M, D, D, SF_EPI_BF16, nullptr, w.a, nullptr), false, s));
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.a, w.vp, params[DH_VP_B], M, D, D, SF_EPI_F32, w.y, nullptr, nullptr), false, s));
  HIP_TRY(sf_launch_layernorm(w.y, params[DH_LN_G], params[DH_LN_B], nullptr, w.ln, nullptr, M, D, eps, s));
  {   // pre = ln fc1^T + b1, act = gelu(pre): one launch where the 256^2 kernel takes the shape
    SfGemmArgs g = sf_train_gemm_args(w.ln, w.fc1, b1, M, Ip, D, SF_EPI_BF16, nullptr, w.pre, nullptr);
    g.aux_mode = 1; g.aux = w.act;
    if (sf_gemm256_aux_supported(g)) {
      HIP_TRY(sf_launch_gemm(g, false, s));
    } else {
      g.aux_mode = 0; g.aux = nullptr;
      HIP_TRY(sf_launch_gemm(g, false, s));
      HIP_TRY(sf_launch_gelu_fwd(w.pre, w.act, (size_t)M * Ip, s));
    }
  }
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.act, w.fc2, params[DH_FC2_B], M, D, Ip, SF_EPI_RESID_F32, out, nullptr, w.y), false, s));
  return SF_OK;
}

static hipError_t dh_wgrad(const DhWs& w, const bf16_t* dy, int ldy, const bf16_t* x, int ldx, int M, int N1, int N2, float* dw, float* db,
                           hipStream_t s) {
  SfWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = dy; a.ldy = ldy; a.x = x; a.ldx = ldx; a.M = M; a.N1 = N1; a.N2 = N2; a.out = dw; a.ldo = N2; a.alpha = 1.f; a.accumulate = 0;
  a.partial = w.wg_partial; a.dbias = db; a.dbias_scratch = w.cs_partial;
  return sf_launch_wgrad(a, s);
}

extern "C" int sf_dense_head_backward(const float* d_out, int M, int D, int I, float eps, const float* const* params, float* d_x,
                                      float* const* grads, void* workspace, size_t workspace_bytes, sf_stream stream) {
  int rc = dh_check("sf_dense_head_backward", M, D, I);
  if (rc) return rc;
  if (!d_out || !params || !d_x || !grads || !workspace) return sf_set_err(SF_ERR_INVALID, "sf_dense_head_backward: null buffer");
  for (int i = 0; i < DH_NPARAM; ++i)
    if (!params[i] || !grads[i]) return sf_set_err(SF_ERR_INVALID, "sf_dense_head_backward: parameter / gradient %d is null", i);
  const DhWs w = dh_carve(workspace, M, D, I);
  if (workspace_bytes < w.bytes) return sf_set_err(SF_ERR_WORKSPACE, "sf_dense_head_backward: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  const int Ip = (I + 63) / 64 * 64;
  // the bias / LayerNorm gradients are accumulated by their kernels: start them at zero (the weight gradients are overwritten)
  const int vec[6] = {DH_WV_B, DH_VP_B, DH_LN_G, DH_LN_B, DH_FC1_B, DH_FC2_B};
  for (int i : vec) HIP_TRY(hipMemsetAsync(grads[i], 0, (size_t)(i == DH_FC1_B ? I : D) * 4, s));
  // out = y + fc2(act)
  HIP_TRY(sf_launch_split(d_out, w.g_bf, nullptr, (size_t)M * D, s));
  {   // d_pre = (g fc2) * gelu'(pre)
    SfGemmArgs g = sf_train_gemm_args(w.g_bf, w.fc2T, nullptr, M, Ip, D, SF_EPI_BF16, nullptr, w.d_wide, nullptr);
    g.aux_mode = 2; g.aux = w.pre;
    if (sf_gemm256_aux_supported(g)) {
      HIP_TRY(sf_launch_gemm(g, false, s));
    } else {
      g.aux_mode = 0; g.aux = nullptr;
      HIP_TRY(sf_launch_gemm(g, false, s));
      HIP_TRY(sf_launch_gelu_bwd(w.d_wide, w.pre, (size_t)M * Ip, s));
    }
  }
  HIP_TRY(dh_wgrad(w, w.g_bf, D, w.act, Ip, M, D, I, grads[DH_FC2_W], grads[DH_FC2_B], s));
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.d_wide, w.fc1T, nullptr, M, D, Ip, SF_EPI_F32, w.d_ln, nullptr, nullptr), false, s));
  HIP_TRY(dh_wgrad(w, w.d_wide, Ip, w.ln, D, M, I, D, grads[DH_FC1_W], grads[DH_FC1_B], s));
  // d_y = d_out + dLayerNorm(y; d_ln), also as the bf16 operand of the next two products
  HIP_TRY(sf_launch_ln_bwd(w.y, w.d_ln, 0, params[DH_LN_G], d_out, w.d_y, w.g_bf, grads[DH_LN_G], grads[DH_LN_B], w.ln_partial, M, D, eps, s));
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.g_bf, w.vpT, nullptr, M, D, D, SF_EPI_BF16, nullptr, w.d_a, nullptr), false, s));
  HIP_TRY(dh_wgrad(w, w.g_bf, D, w.a, D, M, D, D, grads[DH_VP_W], grads[DH_VP_B], s));
  HIP_TRY(sf_launch_gemm(sf_train_gemm_args(w.d_a, w.wvT, nullptr, M, D, D, SF_EPI_F32, d_x, nullptr, nullptr), false, s));
  HIP_TRY(dh_wgrad(w, w.d_a, D, w.xb, D, M, D, D, grads[DH_WV_W], grads[DH_WV_B], s));
  return SF_OK;
}
