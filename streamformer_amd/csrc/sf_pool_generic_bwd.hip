// Pooling head of the training step at generic widths (head_dim != 64, any D = heads * head_dim; SigLIP-so400m: 1152 / 16 = 72).
// The forward is sf_launch_pool_generic (sf_pool_head.hip, bottom): raw scores [F, heads, N] and z [F, heads, D] stay in its scratch for
// the backward here.  Same algebra as the head_dim-64 kernels of sf_pool_head.hip (modeling:1141-1154 with the key / value projections
// folded away: scores = x . U_h, p = softmax, z_h = sum_n p_hn x_n, ctx_h = Wv_h z_h + bv_h), as plain fp32 FMAs:
//   pool_u         U_h = Wk_h^T q_h                                   grid (16, D / 256): a thread per column
//   ctx backward   dz_h = Wv_h^T dctx_h; dWv += dctx^T z; dbv += sum_f dctx      a thread per column, frames in a fixed order
//   probe backward per (frame, head) {max, sum, Delta = dz_h . z_h}; then a wave per token: dp_h = dz_h . x_n,
//                  ds_h = p_hn (dp_h - Delta_h), dx_n = sum_h p_hn dz_h + ds_h U_h (+ the last_hidden_state gradient)
//   U backward     dWk[c] += q[c] dU_h, dq[c] = Wk[c] . dU_h          (h = c / head_dim)
// No atomics, every sum in a fixed order (bit-reproducible).  Functional, not tuned.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_pool_head.h"

__global__ __launch_bounds__(256) void sf_pool_u_gen_kernel(const float* __restrict__ wk, const float* __restrict__ q, float* __restrict__ u,
                                                            int heads, int hd, int D) {
  const int h = blockIdx.x, d = blockIdx.y * 256 + threadIdx.x;
  if (d >= D) return;
  float t = 0.f;
  if (h < heads)
    for (int j = 0; j < hd; ++j) t = fmaf(wk[(size_t)(h * hd + j) * D + d], q[h * hd + j], t);
  u[(size_t)h * D + d] = t;
}
hipError_t sf_launch_pool_u_generic(const float* wk, const float* q, float* u, int heads, int hd, int D, hipStream_t s) {
  if (heads < 1 || heads > 16 || hd < 1 || D != heads * hd) return hipErrorInvalidValue;
  return sf_launch(sf_pool_u_gen_kernel, dim3(16, (D + 255) / 256), dim3(256), 0, s, wk, q, u, heads, hd, D);
}

// dz[f][h][d] = sum_j Wv[h*hd + j][d] dctx[f][h*hd + j]           grid (D / 256, F, heads)
__global__ __launch_bounds__(256) void sf_pool_dz_gen_kernel(const float* __restrict__ dctx, const float* __restrict__ wv, int ldw,
                                                             float* __restrict__ dz, int heads, int hd, int D) {
  const int d = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, h = blockIdx.z;
  if (d >= D) return;
  const float* dr = dctx + (size_t)f * D + h * hd;
  float t = 0.f;
  for (int j = 0; j < hd; ++j) t = fmaf(wv[(size_t)(h * hd + j) * ldw + d], dr[j], t);
  dz[((size_t)f * heads + h) * D + d] = t;
}
// dWv[c][d] += sum_f dctx[f][c] z[f][c / hd][d];  dbv[c] += sum_f dctx[f][c]      grid (D / 256, D rows)
__global__ __launch_bounds__(256) void sf_pool_dwv_gen_kernel(const float* __restrict__ dctx, const float* __restrict__ z, float* __restrict__ dwv,
                                                              int ldw, float* __restrict__ dbv, int F, int heads, int hd, int D) {
  const int d = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, h = c / hd;
  if (d >= D) return;
  float t = 0.f, b = 0.f;
  for (int f = 0; f < F; ++f) {
    const float g = dctx[(size_t)f * D + c];
    t = fmaf(g, z[((size_t)f * heads + h) * D + d], t);
    b += g;
  }
  if (dwv) dwv[(size_t)c * ldw + d] += t;
  if (dbv && d == 0) dbv[c] += b;
}
hipError_t sf_launch_pool_ctx_bwd_generic(const float* dctx, const float* wv, int ldw, const float* z, float* dz, float* dwv, float* dbv, int F,
                                          int heads, int hd, int D, hipStream_t s) {
  if (heads < 1 || heads > 16 || hd < 1 || D != heads * hd || F <= 0) return hipErrorInvalidValue;
  const hipError_t e = sf_launch(sf_pool_dz_gen_kernel, dim3((D + 255) / 256, F, heads), dim3(256), 0, s, dctx, wv, ldw, dz, heads, hd, D);
  if (e != hipSuccess || !(dwv || dbv)) return e;
  return sf_launch(sf_pool_dwv_gen_kernel, dim3((D + 255) / 256, D), dim3(256), 0, s, dctx, z, dwv, ldw, dbv, F, heads, hd, D);
}

// per (frame, head): {max score, sum of exp, Delta = dz_h . z_h}        grid F, a wave per head
__global__ __launch_bounds__(256) void sf_pool_bwd_stats_gen_kernel(SfPoolGenBwdArgs p) {
  const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = wave; h < p.heads; h += 4) {
    const float* sc = p.scores + ((size_t)f * p.heads + h) * p.N;
    float m = -INFINITY;
    for (int n = lane; n < p.N; n += 64) m = fmaxf(m, sc[n]);
    m = wave_max(m);
    float su = 0.f;
    for (int n = lane; n < p.N; n += 64) su += expf(sc[n] - m);
    su = wave_sum(su);
    const float* zr = p.z + ((size_t)f * p.heads + h) * p.D;
    const float* gr = p.dz + ((size_t)f * p.heads + h) * p.D;
    float dl = 0.f;
    for (int d = lane; d < p.D; d += 64) dl = fmaf(gr[d], zr[d], dl);
    dl = wave_sum(dl);
    if (lane == 0) {
      float* o = p.stats + ((size_t)f * p.heads + h) * 4;
      o[0] = m; o[1] = su; o[2] = dl; o[3] = 0.f;
    }
  }
}
// a wave per token: dp, ds (-> ds_bf [M][32], columns >= heads zero), dx                  grid (N / 4, F)
__global__ __launch_bounds__(256) void sf_pool_probe_bwd_gen_kernel(SfPoolGenBwdArgs p) {
  const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= p.N) return;
  const int D = p.D, H = p.heads;
  const size_t tok = (size_t)f * p.N + n;
  const bf16_t* xr = p.x_bf + tok * D;
  float pr[16], ds[16];
#pragma unroll
  for (int h = 0; h < 16; ++h) {
    pr[h] = 0.f; ds[h] = 0.f;
    if (h < H) {
      const float* gr = p.dz + ((size_t)f * H + h) * D;
      float t = 0.f;
      for (int d = lane; d < D; d += 64) t = fmaf(gr[d], bf2f(xr[d]), t);
      t = wave_sum(t);
      const float* st = p.stats + ((size_t)f * H + h) * 4;
      const float pv = expf(p.scores[((size_t)f * H + h) * p.N + n] - st[0]) / st[1];
      pr[h] = pv;
      ds[h] = pv * (t - st[2]);
    }
  }
  if (lane < 32) {
    float v = 0.f;
#pragma unroll
    for (int h = 0; h < 16; ++h) v = lane == h ? ds[h] : v;
    p.ds_bf[tok * 32 + lane] = (bf16_t)f2bf(v);
  }
  float* dxr = p.dx + tok * D;
  const float* lr = p.d_lhs ? p.d_lhs + tok * D : nullptr;
  for (int d = lane; d < D; d += 64) {
    float t = lr ? lr[d] : 0.f;
#pragma unroll
    for (int h = 0; h < 16; ++h)
      if (h < H) {
        t = fmaf(pr[h], p.dz[((size_t)f * H + h) * D + d], t);
        t = fmaf(ds[h], p.u[(size_t)h * D + d], t);
      }
    dxr[d] = t;
  }
}
hipError_t sf_launch_pool_probe_bwd_generic(const SfPoolGenBwdArgs& a, hipStream_t s) {
  if (a.heads < 1 || a.heads > 16 || a.F <= 0 || a.N <= 0 || a.D <= 0 || !a.stats) return hipErrorInvalidValue;
  const hipError_t e = sf_launch(sf_pool_bwd_stats_gen_kernel, dim3(a.F), dim3(256), 0, s, a);
  if (e != hipSuccess) return e;
  return sf_launch(sf_pool_probe_bwd_gen_kernel, dim3((a.N + 3) / 4, a.F), dim3(256), 0, s, a);
}

// dWk[c][d] += q[c] dU[h][d];  dq[c] = sum_d Wk[c][d] dU[h][d]   (h = c / hd; grid D rows)
__global__ __launch_bounds__(256) void sf_pool_u_bwd_gen_kernel(const float* __restrict__ du, const float* __restrict__ wk, const float* __restrict__ q,
                                                                float* __restrict__ dwk, float* __restrict__ dq, int hd, int D) {
  __shared__ float red[4];
  const int c = blockIdx.x, h = c / hd, tid = threadIdx.x;
  const float qc = q[c];
  float t = 0.f;
  for (int d = tid; d < D; d += 256) {
    const float g = du[(size_t)h * D + d];
    t = fmaf(wk[(size_t)c * D + d], g, t);
    if (dwk) dwk[(size_t)c * D + d] += qc * g;
  }
  t = wave_sum(t);
  if ((tid & 63) == 0) red[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) dq[c] = (red[0] + red[1]) + (red[2] + red[3]);
}
hipError_t sf_launch_pool_u_bwd_generic(const float* du, const float* wk, const float* q, float* dwk, float* dq, int hd, int D, hipStream_t s) {
  if (hd < 1 || D % hd) return hipErrorInvalidValue;
  return sf_launch(sf_pool_u_bwd_gen_kernel, dim3(D), dim3(256), 0, s, du, wk, q, dwk, dq, hd, D);
}
