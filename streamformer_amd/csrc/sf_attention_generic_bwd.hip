// Attention backward for head widths the tuned kernels of sf_attention_bwd.hip (head_dim 64) do not cover: any head_dim that is a
// multiple of 8 up to 128 (SigLIP-so400m: 1152 / 16 = 72), spatial L <= 224, temporal L <= 32 (causal or not).  Same SfAttnBwdArgs
// contract as sf_launch_spatial_attention_bwd / sf_launch_temporal_attention_bwd, plus `head_dim`.
//
// One workgroup (4 waves) per (sequence, head); everything in fp32 from bf16 operands staged in LDS as [L][head_dim + 2] bf16 rows
// (pitch of head_dim / 2 + 1 words: odd, so the lanes of a wave that walk different rows at the same column hit different banks).
//   phase A + C  (K | V staged)   a wave per query row i: s_ij = scale q_i . k_j and dp_ij = dO_i . v_j with lanes over the keys,
//                                 lse_i / Delta_i = dO_i . o_i, dS_ij = P_ij (dp_ij - Delta_i) into a wave-private row, then
//                                 dQ_i = scale sum_j dS_ij k_j with lanes over the columns
//   phase B      (Q | dO staged)  a wave per key row j: P_ij, dS_ij recomputed from the saved lse_i / Delta_i with lanes over the queries,
//                                 dV_j = sum_i P_ij dO_i, dK_j = scale sum_i dS_ij q_i with lanes over the columns
// Every output element has one owner and every sum a fixed order: bit-reproducible, no atomics.  No log-sum-exp input (the
// statistics are recomputed) and no attention-probability dropout.  A functional path, not a tuned one: plain FMAs, one workgroup of
// <= 130 KB LDS per problem.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_train.h"

#include <cmath>

#define GB_WAVES 4

struct GbView {
  const unsigned* x0;     // staged rows [L][pw] words (bf16 pairs): K (phase A / C) or Q (phase B)
  const unsigned* x1;     //                                         V                 dO
  int pw;                 // row pitch in 32-bit words: head_dim / 2 + 1
  int hw;                 // head_dim / 2
};

// a . r over the head_dim columns: a fp32 [head_dim] (wave-uniform, LDS broadcast), r a staged bf16 row
SF_DEVICE float gb_dot(const float* a, const unsigned* r, int hw) {
  float t = 0.f;
  for (int c = 0; c < hw; ++c) {
    const unsigned w = r[c];
    t = fmaf(a[2 * c], bf2f(w & 0xffffu), t);
    t = fmaf(a[2 * c + 1], __uint_as_float(w & 0xffff0000u), t);
  }
  return t;
}

// element d of a staged row
SF_DEVICE float gb_el(const unsigned* r, int d) {
  const unsigned w = r[d >> 1];
  return (d & 1) ? __uint_as_float(w & 0xffff0000u) : bf2f(w & 0xffffu);
}

SF_DEVICE void gb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * GB_WAVES) void sf_attention_generic_bwd_kernel(SfAttnBwdArgs a, int temporal) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hd = a.head_dim, hw = hd >> 1, pw = hw + 1, L = a.L;
  const int h = blockIdx.x % a.heads, seq = blockIdx.x / a.heads;
  long row_base, row_step;
  if (temporal) { row_base = (long)(seq / a.seq_rows) * L * a.seq_rows + seq % a.seq_rows; row_step = a.seq_rows; }
  else { row_base = (long)seq * L; row_step = 1; }
  auto row = [&](int t) { return (size_t)(row_base + (long)t * row_step); };

  unsigned* x0 = reinterpret_cast<unsigned*>(smem);
  unsigned* x1 = x0 + (size_t)L * pw;
  float* lse = reinterpret_cast<float*>(x1 + (size_t)L * pw);
  float* delta = lse + L;
  float* wbase = delta + L;
  const int per_wave = 2 * 128 + 2 * L;       // two fp32 vectors of the row, two weight rows over the sequence
  float* va = wbase + wave * per_wave;
  float* vb = va + 128;
  float* w0 = vb + 128;
  float* w1 = w0 + L;

  auto stage = [&](const bf16_t* src0, int ld0, const bf16_t* src1, int ld1) {
    for (int e = tid; e < L * hw; e += 64 * GB_WAVES) {
      const int r = e / hw, c = e % hw;
      x0[r * pw + c] = *reinterpret_cast<const unsigned*>(src0 + row(r) * ld0 + 2 * c);
      x1[r * pw + c] = *reinterpret_cast<const unsigned*>(src1 + row(r) * ld1 + 2 * c);
    }
  };
  const bf16_t* qg = a.qkv + (size_t)h * hd;
  const bf16_t* kg = qg + a.D;
  const bf16_t* vg = qg + 2 * a.D;
  const bf16_t* og = a.o + (size_t)h * hd;
  const bf16_t* gg = a.d_o + (size_t)h * hd;
  bf16_t* dq = a.d_qkv + (size_t)h * hd;
  bf16_t* dk = dq + a.D;
  bf16_t* dv = dq + 2 * a.D;

  // ---- phase A + C: row statistics, Delta, dQ (K | V staged) ---------------------------------------------------------------
  stage(kg, a.ld_qkv, vg, a.ld_qkv);
  __syncthreads();
  for (int i = wave; i < L; i += GB_WAVES) {
    const size_t ri = row(i);
    float dl = 0.f;
    for (int d = lane; d < hd; d += 64) {
      va[d] = bf2f(qg[ri * a.ld_qkv + d]);
      const float gd = bf2f(gg[ri * a.ld_o + d]);
      vb[d] = gd;
      dl = fmaf(gd, bf2f(og[ri * a.ld_o + d]), dl);
    }
    dl = wave_sum(dl);
    gb_wave_sync();
    const int jn = a.causal ? i + 1 : L;
    float s[4], dp[4];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      s[k] = -INFINITY; dp[k] = 0.f;
      if (j < jn) {
        s[k] = a.scale * gb_dot(va, x0 + j * pw, hw);
        dp[k] = gb_dot(vb, x1 + j * pw, hw);
      }
      m = fmaxf(m, s[k]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += (lane + 64 * k < jn) ? expf(s[k] - m) : 0.f;
    sum = wave_sum(sum);
    const float ls = m + logf(sum);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      if (j < L) w0[j] = j < jn ? expf(s[k] - ls) * (dp[k] - dl) : 0.f;
    }
    if (lane == 0) { lse[i] = ls; delta[i] = dl; }
    gb_wave_sync();
    for (int d = lane; d < hd; d += 64) {
      float t = 0.f;
      for (int j = 0; j < jn; ++j) t = fmaf(w0[j], gb_el(x0 + j * pw, d), t);
      dq[ri * a.ld_qkv + d] = (bf16_t)f2bf(a.scale * t);
    }
    gb_wave_sync();
  }
  __syncthreads();

  // ---- phase B: dK, dV per key row (Q | dO staged) --------------------------------------------------------------------------
  stage(qg, a.ld_qkv, gg, a.ld_o);
  __syncthreads();
  for (int j = wave; j < L; j += GB_WAVES) {
    const size_t rj = row(j);
    for (int d = lane; d < hd; d += 64) {
      va[d] = bf2f(kg[rj * a.ld_qkv + d]);
      vb[d] = bf2f(vg[rj * a.ld_qkv + d]);
    }
    gb_wave_sync();
    const int i0 = a.causal ? j : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lane + 64 * k;
      if (i < L) {
        float p = 0.f, ds = 0.f;
        if (i >= i0) {
          p = expf(a.scale * gb_dot(va, x0 + i * pw, hw) - lse[i]);
          ds = p * (gb_dot(vb, x1 + i * pw, hw) - delta[i]);
        }
        w0[i] = p; w1[i] = ds;
      }
    }
    gb_wave_sync();
    for (int d = lane; d < hd; d += 64) {
      float tv = 0.f, tk = 0.f;
      for (int i = i0; i < L; ++i) {
        tv = fmaf(w0[i], gb_el(x1 + i * pw, d), tv);
        tk = fmaf(w1[i], gb_el(x0 + i * pw, d), tk);
      }
      dv[rj * a.ld_qkv + d] = (bf16_t)f2bf(tv);
      dk[rj * a.ld_qkv + d] = (bf16_t)f2bf(a.scale * tk);
    }
    gb_wave_sync();
  }
}

static size_t gb_lds(int L, int hd) {
  return (size_t)2 * L * (hd / 2 + 1) * 4 + (size_t)2 * L * 4 + (size_t)GB_WAVES * (2 * 128 + 2 * L) * 4;
}

hipError_t sf_launch_attention_generic_bwd(const SfAttnBwdArgs& a, bool temporal, hipStream_t s) {
  const int hd = a.head_dim;
  if (hd < 8 || hd > 128 || hd % 8 || a.D != a.heads * hd || a.L <= 0 || a.nseq <= 0 || a.heads <= 0) return hipErrorInvalidValue;
  if (a.L > (temporal ? 32 : 224) || (temporal && a.seq_rows <= 0) || a.drop.on) return hipErrorInvalidValue;
  if ((a.ld_qkv % 2) || (a.ld_o % 2)) return hipErrorInvalidValue;
  const size_t lds = gb_lds(a.L, hd);       // <= 129.8 KB at L = 224, head_dim 128
  return sf_launch_big_lds(sf_attention_generic_bwd_kernel, dim3(a.nseq * a.heads), dim3(64 * GB_WAVES), lds, s, a, temporal ? 1 : 0);
}
