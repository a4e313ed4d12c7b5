// Temporal attention, head_dim 64 (gfx950, MFMA 16x16x32 bf16): softmax(q k^T d^-0.5) v over the frames of one patch, causal, over a
// KV-cache (reference modeling:575-615; streaming copy vqa_enc:491-560: cache append, offset causal mask).  Row addressing: see SfAttnArgs.
//   sf_temporal_attn_dma_kernel  Tq <= 16 queries against Tk <= 32 frames (every full clip): 128-byte-row images by LDS-DMA (sf_attn_image.h)
//   sf_temporal_attn_kernel      long caches, fp32 rows, T_new > 16: register-staged, the score layout of the staged spatial kernel
// and the route: sf_temporal_route() decides for every temporal call, the single-query (Tq = 1) ones included, whose kernels live in
// sf_attention_decode.hip; sf_launch_temporal_route() launches.
#include "sf_attention_fwd.h"

static int vt_pitch(int nkp) {
  // bytes per V^T row: 2*nkp + pad with pitch % 256 in {32, 224}: the 16 d-rows of a ds_read_b128
  // lane group then fall on 16 distinct 16-byte slots ("LDS layouts").
  for (int pad = 0; pad < 256; pad += 32) {
    const int m = (2 * nkp + pad) % 256;
    if (m == 32 || m == 224) return 2 * nkp + pad;
  }
  return 2 * nkp + 32;
}
// ================================================================================================
// Register-staged kernel: ONE WAVE per (b, patch, head) task, four consecutive tasks (adjacent heads =
// adjacent 128-byte lines) per workgroup, no workgroup barrier.  Every global load of the task
// (Q, K fragments, V rows) is issued up front so a task costs one memory latency; V^T goes through
// a wave-private LDS patch, the context rows leave as whole 128-byte segments.
// Swapped QK^T, permuted K rows and the ACC scheme: as the staged kernel of sf_attention_spatial.hip.
// ================================================================================================
template <bool ACC, int MAXNT2>
__global__ __launch_bounds__(256) void sf_temporal_attn_kernel(SfAttnArgs p, int vpitch, int ntasks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool PRELOAD_K = MAXNT2 <= 2;          // K fragments of the whole key range live in registers
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int task = blockIdx.x * (blockDim.x >> 6) + wave;
  if (task >= ntasks) return;
  const int h = task % p.heads, bn = task / p.heads;
  const int b = bn / p.N, n = bn % p.N;
  const int Tk = p.Tk, Tq = p.Tq;
  const int tkp = (Tk + 31) & ~31;
  const int nt2 = tkp >> 5;
  const int patch = HD * vpitch * (ACC ? 2 : 1) + (ACC ? 4096 : 2048);
  char* v_hi = smem + (size_t)wave * patch;
  char* v_lo = v_hi + (ACC ? HD * vpitch : 0);
  char* o_st = v_lo + HD * vpitch;

  // ---- issue every load of the task ------------------------------------------------------------------
  bf16x8_t qh[2], ql[2];
  {
    int t = l15 < Tq ? l15 : Tq - 1;
    const size_t qrow = ((size_t)b * p.Tq_cap + p.q_t0 + t) * p.N + n;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) load_frag<ACC>(p.q, qrow * p.row_pitch_q + h * HD + ks * 32 + g * 8, qh[ks], ql[ks]);
  }
  bf16x8_t kfh[PRELOAD_K ? MAXNT2 : 1][2][2], kfl[PRELOAD_K ? MAXNT2 : 1][2][2];
  if (PRELOAD_K) {
#pragma unroll
    for (int kt2 = 0; kt2 < MAXNT2; ++kt2)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        int key = kt2 * 32 + (l15 >> 2) * 8 + hh * 4 + (l15 & 3);
        key = key < Tk ? key : Tk - 1;                     // clamped rows are masked below
        const size_t krow = ((size_t)b * p.Tcap + key) * p.N + n;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          load_frag<ACC>(p.k, krow * p.row_pitch_kv + h * HD + ks * 32 + g * 8, kfh[kt2][hh][ks], kfl[kt2][hh][ks]);
      }
  }
  // V rows -> V^T patch: item = (key pair, 8-wide d chunk)
  for (int i = lane; i < (tkp >> 1) * 8; i += 64) {
    const int kp = i >> 3, c = i & 7;
    float v0[8], v1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { v0[j] = 0.f; v1[j] = 0.f; }
    if (2 * kp < Tk) load8<ACC>(p.v, (((size_t)b * p.Tcap + 2 * kp) * p.N + n) * p.row_pitch_kv + h * HD + c * 8, v0);
    if (2 * kp + 1 < Tk) load8<ACC>(p.v, (((size_t)b * p.Tcap + 2 * kp + 1) * p.N + n) * p.row_pitch_kv + h * HD + c * 8, v1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned int h0, l0, h1, l1;
      split_bf(v0[j], h0, l0);
      split_bf(v1[j], h1, l1);
      const int off = (c * 8 + j) * vpitch + kp * 4;
      *reinterpret_cast<unsigned int*>(v_hi + off) = h0 | (h1 << 16);
      if (ACC) *reinterpret_cast<unsigned int*>(v_lo + off) = l0 | (l1 << 16);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int nqt = (Tq + 15) >> 4;
  for (int qt = 0; qt < nqt; ++qt) {
    int t = qt * 16 + l15;
    const bool qvalid = t < Tq;
    if (!qvalid) t = Tq - 1;
    if (qt > 0) {      // further query tiles (T_new > 16): reload Q
      const size_t qrow = ((size_t)b * p.Tq_cap + p.q_t0 + t) * p.N + n;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) load_frag<ACC>(p.q, qrow * p.row_pitch_q + h * HD + ks * 32 + g * 8, qh[ks], ql[ks]);
    }
    f32x4_t s[MAXNT2][2];
#pragma unroll
    for (int kt2 = 0; kt2 < MAXNT2; ++kt2) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        if (kt2 < nt2) {
          int key = kt2 * 32 + (l15 >> 2) * 8 + hh * 4 + (l15 & 3);
          key = key < Tk ? key : Tk - 1;
          const size_t krow = ((size_t)b * p.Tcap + key) * p.N + n;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t kh, kl;
            if (PRELOAD_K) { kh = kfh[kt2][hh][ks]; kl = kfl[kt2][hh][ks]; }
            else load_frag<ACC>(p.k, krow * p.row_pitch_kv + h * HD + ks * 32 + g * 8, kh, kl);
            if (ACC) {
              acc = mfma16(kl, qh[ks], acc);
              acc = mfma16(kh, ql[ks], acc);
            }
            acc = mfma16(kh, qh[ks], acc);
          }
        }
        s[kt2][hh] = acc;
      }
    }
    const int qpos = p.t_past + t;   // absolute frame index of this lane's query
    const int causal = p.causal;
    const float sum = softmax_tiles<ACC, MAXNT2>(s, nt2, g, p.scale, 0,
                                                 [&](int, int key) { return key < Tk && (!causal || key <= qpos); });
    const float inv = 1.0f / sum;

    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt2 = 0; kt2 < MAXNT2; ++kt2) {
      if (kt2 < nt2) {
        bf16x8_t ph, pl;
        pack_p<ACC>(s[kt2][0], s[kt2][1], ph, pl);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int off = (dt * 16 + l15) * vpitch + (kt2 * 32 + g * 8) * 2;
          const bf16x8_t vh = *reinterpret_cast<const bf16x8_t*>(v_hi + off);
          if (ACC) {
            const bf16x8_t vl = *reinterpret_cast<const bf16x8_t*>(v_lo + off);
            o[dt] = mfma16(vl, ph, o[dt]);
            o[dt] = mfma16(vh, pl, o[dt]);
          }
          o[dt] = mfma16(vh, ph, o[dt]);
        }
      }
    }
    // ---- context: lane holds d = dt*16 + g*4..+4 of query l15 -> wave patch -> 128-byte row segments
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      unsigned int hb[4], lb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) split_bf(o[dt][j] * inv, hb[j], lb[j]);
      const int off = l15 * 128 + (((dt * 2 + (g >> 1)) ^ (l15 & 7)) << 4) + (g & 1) * 8;
      *reinterpret_cast<u32x2_t*>(o_st + off) = (u32x2_t){hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16)};
      if (ACC) *reinterpret_cast<u32x2_t*>(o_st + 2048 + off) = (u32x2_t){lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16)};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = it * 64 + lane;
      const int r = idx >> 3, c = idx & 7;
      const int tq = qt * 16 + r;
      if (tq < Tq) {
        const size_t o_off = (((size_t)b * Tq + tq) * p.N + n) * p.D + h * HD + c * 8;
        const int off = r * 128 + ((c ^ (r & 7)) << 4);
        *reinterpret_cast<u32x4_t*>(p.ctx_hi + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + off);
        if (ACC) *reinterpret_cast<u32x4_t*>(p.ctx_lo + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + 2048 + off);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ================================================================================================
// temporal attention, bf16 mode, short sequences (Tq <= 16 queries against Tk <= 32 cached frames: every full 16-frame
// clip): the round-2 staging of the spatial kernel applied to the per-(patch, head) problem.  One wave per task; K and
// V rows (one 128-byte line per frame) go global -> LDS by LDS-DMA as row-major images, K fragments are plain row reads,
// V^T fragments transposed reads (ds_read_b64_tr_b16), natural key order, P stays in registers.  The MFMA kernel above
// keeps the long caches, the accurate mode and T_new > 16.
// ================================================================================================
// ACC: hi + lo bf16 planes of q / k / v (the accurate mode's full-clip forward writes them instead of fp32), four images per
// wave, three MFMAs per product, probabilities and context split into hi + lo in registers.
template <bool ACC>
__global__ __launch_bounds__(256) void sf_temporal_attn_dma_kernel(SfAttnArgs p, int ntasks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int task = blockIdx.x * 4 + wave;
  if (task >= ntasks) return;
  const int h = task % p.heads, bn = task / p.heads;
  const int b = bn / p.N, n = bn % p.N;
  const int Tk = p.Tk, Tq = p.Tq;
  char* k_img = smem + wave * (ACC ? 20480 : 10240);          // [32 rows][128 B]
  char* v_img = k_img + 4096;                 // [32 rows][128 B]
  char* o_st = v_img + 4096;                  // [16 rows][128 B] (hi; ACC: lo at + 2048 ... see below)
  char* kl_img = o_st + (ACC ? 4096 : 2048);  // ACC only
  char* vl_img = kl_img + 4096;
  const bf16_t* kbase = reinterpret_cast<const bf16_t*>(p.k) + h * HD;
  const bf16_t* vbase = reinterpret_cast<const bf16_t*>(p.v) + h * HD;
#pragma unroll
  for (int j = 0; j < 4; ++j) {               // instruction j covers frames 8j .. 8j+7
    const int row = j * 8 + (lane >> 3);
    const int chunk = img_dma_chunk(lane, row);
    const int key = row < Tk ? row : Tk - 1;  // padding rows repeat the last frame (masked below)
    const size_t src = (((size_t)b * p.Tcap + key) * p.N + n) * (size_t)p.row_pitch_kv + chunk * 8;
    __builtin_amdgcn_global_load_lds((dma_gptr_t)(kbase + src), (dma_lptr_t)(k_img + j * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((dma_gptr_t)(vbase + src), (dma_lptr_t)(v_img + j * 1024), 16, 0, 0);
    if (ACC) {
      __builtin_amdgcn_global_load_lds((dma_gptr_t)(kbase + p.lo_plane_off + src), (dma_lptr_t)(kl_img + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((dma_gptr_t)(vbase + p.lo_plane_off + src), (dma_lptr_t)(vl_img + j * 1024), 16, 0, 0);
    }
  }
  bf16x8_t qf[2], ql[2];
  {
    const int t = l15 < Tq ? l15 : Tq - 1;
    const size_t qrow = ((size_t)b * p.Tq_cap + p.q_t0 + t) * p.N + n;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16_t* qp = reinterpret_cast<const bf16_t*>(p.q) + qrow * p.row_pitch_q + h * HD + ks * 32 + g * 8;
      qf[ks] = *reinterpret_cast<const bf16x8_t*>(qp);
      if (ACC) ql[ks] = *reinterpret_cast<const bf16x8_t*>(qp + p.lo_plane_off);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();            // the images are wave-private: no workgroup barrier
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // S^T = K Q^T: lane (query l15, g) holds keys 16 jt + 4 g + r
  f32x4_t s[2];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8_t kh = row_frag(k_img, jt * 16 + l15, ks * 4 + g);
      if (ACC) {
        acc = mfma16(row_frag(kl_img, jt * 16 + l15, ks * 4 + g), qf[ks], acc);
        acc = mfma16(kh, ql[ks], acc);
      }
      acc = mfma16(kh, qf[ks], acc);
    }
    s[jt] = acc;
  }
  __builtin_amdgcn_sched_barrier(0);          // mask / maximum only after both tiles' MFMAs (see the spatial kernel)
  const int qpos = p.t_past + l15;            // absolute frame of this lane's query
  const int causal = p.causal;
  float mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = jt * 16 + 4 * g + r;
      const bool ok = key < Tk && (!causal || key <= qpos);
      s[jt][r] = ok ? s[jt][r] : -INFINITY;
      mx = fmaxf(mx, s[jt][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float c2 = p.scale * 1.44269504088896340736f;
  const float mc = mx * c2;
  float sum = 0.f;
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __builtin_amdgcn_exp2f(fmaf(s[jt][r], c2, -mc));
      s[jt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  if (p.drop.on) {      // training: dropout on the (normalised) probabilities (modeling:603) — the denominator above is unmasked
    const unsigned dbase = (unsigned)((((size_t)bn * p.heads + h) * Tq + (l15 < Tq ? l15 : Tq - 1)) * Tk);
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[jt][r] *= sf_drop_factor(p.drop, dbase + (unsigned)(jt * 16 + 4 * g + r));
  }
  const u32x4_t pu = {pack_bf2(s[0][0], s[0][1]), pack_bf2(s[0][2], s[0][3]), pack_bf2(s[1][0], s[1][1]), pack_bf2(s[1][2], s[1][3])};
  const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pu);
  bf16x8_t pl;
  if (ACC) {
    u32x4_t lu;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const f32x4_t& sv = s[w >> 1];
      const int r0 = (w & 1) * 2;
      lu[w] = pack_bf2(sv[r0] - bf2f(pu[w] & 0xffffu), sv[r0 + 1] - bf2f(pu[w] >> 16));
    }
    pl = __builtin_bit_cast(bf16x8_t, lu);
  }
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const bf16x8_t vh = tr_frag<true>(v_img, 0, dt, lane);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    if (ACC) {
      acc = mfma16(tr_frag<true>(vl_img, 0, dt, lane), pf, acc);
      acc = mfma16(vh, pl, acc);
    }
    o[dt] = mfma16(vh, pf, acc);
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int off = l15 * 128 + (((dt * 2 + (g >> 1)) ^ (l15 & 7)) << 4) + (g & 1) * 8;
    const f32x4_t ov = o[dt] * inv;
    const u32x2_t hv = {pack_bf2(ov[0], ov[1]), pack_bf2(ov[2], ov[3])};
    *reinterpret_cast<u32x2_t*>(o_st + off) = hv;
    if (ACC)
      *reinterpret_cast<u32x2_t*>(o_st + 2048 + off) = (u32x2_t){pack_bf2(ov[0] - bf2f(hv[0] & 0xffffu), ov[1] - bf2f(hv[0] >> 16)),
                                                                pack_bf2(ov[2] - bf2f(hv[1] & 0xffffu), ov[3] - bf2f(hv[1] >> 16))};
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = it * 64 + lane;
    const int r = idx >> 3, c = idx & 7;
    if (r < Tq) {
      const size_t oo = (((size_t)b * Tq + r) * p.N + n) * p.D + h * HD + c * 8;
      *reinterpret_cast<u32x4_t*>(p.ctx_hi + oo) = *reinterpret_cast<const u32x4_t*>(o_st + r * 128 + ((c ^ (r & 7)) << 4));
      if (ACC) *reinterpret_cast<u32x4_t*>(p.ctx_lo + oo) = *reinterpret_cast<const u32x4_t*>(o_st + 2048 + r * 128 + ((c ^ (r & 7)) << 4));
    }
  }
}
// accurate mode: may the caller hand q / k / v of the temporal attention as hi + lo bf16 planes (short clips, no cache)?
bool sf_temporal_planes_ok(int Tq, int Tk) {
  const bool off = sf_sw(SW_DISABLE_TEMPORAL_DMA_ACC) != nullptr || sf_sw(SW_DISABLE_TEMPORAL_DMA) != nullptr;
  return !off && Tq > 1 && Tq <= 16 && Tk <= 32;
}

// What sf_launch_temporal_attention runs for a call: decided here, launched by sf_launch_temporal_route (nothing else chooses a kernel).
SfTemporalRoute sf_temporal_route(const SfAttnArgs& a, bool accurate) {
  if (a.head_dim && a.head_dim != HD)                // sf_attention_generic.hip
    return sf_attention_generic_supported(a, a.head_dim) && a.B > 0 && a.N > 0 && a.Tq > 0 && a.Tk > 0 && !a.probs ? SF_TROUTE_GENERIC : SF_TROUTE_NONE;
  if (a.D != a.heads * HD || a.Tq <= 0 || a.Tk <= 0 || a.B <= 0 || a.N <= 0) return SF_TROUTE_NONE;
  // dropout on the probabilities (training forward): the DMA-staged whole-clip kernel only
  if (a.drop.on && (accurate || a.Tq == 1 || a.Tq > 16 || a.Tk > 32 || (a.row_pitch_kv % 8) || sf_sw(SW_DISABLE_TEMPORAL_DMA))) return SF_TROUTE_NONE;
  const bool decode_off = sf_sw(SW_DISABLE_TEMPORAL_DECODE) != nullptr;
  if (a.Tq == 1 && a.Tk <= 256 && !decode_off) {        // one new frame per stream: the matrix-vector kernel
    const int kp = (a.Tk + 63) >> 6;
    if (accurate) return kp <= 1 ? SF_TROUTE_DECODE_F32_KP1 : kp <= 2 ? SF_TROUTE_DECODE_F32_KP2 : SF_TROUTE_DECODE_F32_KP4;
    // bf16 rows, <= 128 keys: whole cache lines per load instruction
    if (kp <= 2 && (a.row_pitch_kv % 8) == 0 && (a.row_pitch_q % 8) == 0 && !sf_sw(SW_TEMPORAL_DECODE_LANE_KEY))
      return kp <= 1 ? SF_TROUTE_DECODE_LINES_KP1 : SF_TROUTE_DECODE_LINES_KP2;
    return kp <= 1 ? SF_TROUTE_DECODE_BF16_KP1 : kp <= 2 ? SF_TROUTE_DECODE_BF16_KP2 : SF_TROUTE_DECODE_BF16_KP4;
  }
  const bool tdma_off = sf_sw(SW_DISABLE_TEMPORAL_DMA) != nullptr;
  if (!accurate && !tdma_off && a.Tq <= 16 && a.Tk <= 32 && (a.row_pitch_kv % 8) == 0) return SF_TROUTE_DMA_BF16;     // every full 16-frame clip
  if (accurate && !a.in_is_f32)          // hi + lo planes (sf_temporal_planes_ok)
    return a.Tq > 16 || a.Tk > 32 || a.lo_plane_off <= 0 || (a.row_pitch_kv % 8) || (a.lo_plane_off % 8) ? SF_TROUTE_NONE : SF_TROUTE_DMA_PLANES;
  const int tkp = (a.Tk + 31) & ~31;
  if (tkp > 32 * 8) return SF_TROUTE_NONE;   // <= 256 cached frames per stream
  const int nt2 = tkp >> 5;
  const int step = nt2 <= 1 ? 0 : nt2 <= 2 ? 1 : nt2 <= 4 ? 2 : 3;
  return (SfTemporalRoute)((accurate ? SF_TROUTE_MFMA_ACC_NT1 : SF_TROUTE_MFMA_BF16_NT1) + step);
}

static bool troute_mfma(SfTemporalRoute r) { return r >= SF_TROUTE_MFMA_ACC_NT1 && r <= SF_TROUTE_MFMA_BF16_NT8; }
static size_t troute_mfma_patch(SfTemporalRoute r, const SfAttnArgs& a) {      // LDS bytes per wave of the MFMA routes
  const bool accurate = r <= SF_TROUTE_MFMA_ACC_NT8;
  return (size_t)HD * vt_pitch((a.Tk + 31) & ~31) * (accurate ? 2 : 1) + (accurate ? 4096 : 2048);
}
int sf_temporal_route_waves(SfTemporalRoute r, const SfAttnArgs& a) {
  if (!troute_mfma(r)) return 4;
  const size_t patch = troute_mfma_patch(r, a);
  int waves = 4;
  while (waves > 1 && patch * waves > 150 * 1024) waves >>= 1;
  return waves;
}

hipError_t sf_launch_temporal_route(SfTemporalRoute r, const SfAttnArgs& a, hipStream_t s) {
  if (r == SF_TROUTE_NONE) return hipErrorInvalidValue;
  if (r == SF_TROUTE_GENERIC) return sf_launch_attention_generic(a, a.head_dim, true, s);
  const int ntasks = a.B * a.N * a.heads;
  if (troute_mfma(r)) {
    const int vp = vt_pitch((a.Tk + 31) & ~31);
    const int waves = sf_temporal_route_waves(r, a);
    const size_t lds = troute_mfma_patch(r, a) * waves;
    const dim3 grid((ntasks + waves - 1) / waves), block(waves * 64);
#define SF_TL(ACCV, NT) return sf_launch_big_lds(sf_temporal_attn_kernel<ACCV, NT>, grid, block, lds, s, a, vp, ntasks)
    switch (r) {
      case SF_TROUTE_MFMA_ACC_NT1: SF_TL(true, 1);
      case SF_TROUTE_MFMA_ACC_NT2: SF_TL(true, 2);
      case SF_TROUTE_MFMA_ACC_NT4: SF_TL(true, 4);
      case SF_TROUTE_MFMA_ACC_NT8: SF_TL(true, 8);
      case SF_TROUTE_MFMA_BF16_NT1: SF_TL(false, 1);
      case SF_TROUTE_MFMA_BF16_NT2: SF_TL(false, 2);
      case SF_TROUTE_MFMA_BF16_NT4: SF_TL(false, 4);
      default: SF_TL(false, 8);
    }
#undef SF_TL
  }
  const dim3 grid((ntasks + 3) / 4), block(256);
  switch (r) {
    case SF_TROUTE_DMA_BF16: return sf_launch(sf_temporal_attn_dma_kernel<false>, grid, block, 4 * 10240, s, a, ntasks);
    case SF_TROUTE_DMA_PLANES: return sf_launch_big_lds(sf_temporal_attn_dma_kernel<true>, grid, block, 4 * 20480, s, a, ntasks);
    default: return sf_launch_temporal_decode(r, a, s);      // the single-query routes (sf_attention_decode.hip)
  }
}

hipError_t sf_launch_temporal_attention(const SfAttnArgs& a, bool accurate, hipStream_t s) {
  return sf_launch_temporal_route(sf_temporal_route(a, accurate), a, s);
}
