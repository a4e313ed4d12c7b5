// Temporal attention of ONE new frame per stream, head_dim 64 (Tq = 1: the streaming step, vqa_enc:1316-1392 with a single-frame call):
// a matrix-vector problem per (b, patch, head) — q (64) against Tk cached keys — so there is nothing for the MFMA to do.  Two kernels,
// one wave per task, plain VALU, no LDS, no barrier; sf_temporal_route() (sf_attention_temporal.hip) chooses between them and
// sf_launch_temporal_decode() at the end of this file launches.
//
// sf_temporal_decode_kernel (fp32 or bf16 rows, <= 256 keys):
//   scores : lane = key (KP passes of 64 keys); the lane reads its key row (128 B bf16 / 256 B fp32) and dots it
//            with q in fp32 (exact products of the stored operands; the fp32-accurate mode needs no bf16x3 here);
//   softmax: two wave reductions (max, sum);
//   P V    : lane = (key mod 8, 8-wide d chunk): eight keys x 128 B per load instruction (whole lines), the lane's
//            probability comes by ds_bpermute, partial rows meet by three xor-shuffles per value.
// Every load of the task is issued before the first use (one memory latency per task).
// The MFMA kernel pays ~10-17 us per launch at one frame (V^T staging through LDS, 16-query tiles with one
// live query); this one is bound by the cache read: Tk x 196 x 768 x 2 x 2 B.
#include "sf_attention_fwd.h"

template <bool F32, int KP>
__global__ __launch_bounds__(256) void sf_temporal_decode_kernel(SfAttnArgs p, int ntasks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int task = blockIdx.x * 4 + wave;
  if (task >= ntasks) return;
  const int h = task % p.heads, bn = task / p.heads;
  const int b = bn / p.N, n = bn % p.N;
  // the cache position by value, or (streamed frame replayed from the position-free graph) from device memory
  // (ragged call: this sequence's own entry of the call's table, and its cache slab bs; the context row stays row b)
  int q_t0 = p.q_t0, Tk = p.Tk, bs = b;
  if (p.tab) {
    const SfStreamSlot e = p.tab[b];
    bs = e.stream; q_t0 = e.slot; Tk = min(e.tk, KP * 64);
  } else if (p.pos_dev) {
    q_t0 = p.pos_dev[0]; Tk = min(p.pos_dev[1], KP * 64);
  }
  const int t_past = (p.tab || p.pos_dev) ? Tk - 1 : p.t_past;         // absolute index of the query among the keys (causal: keys <= it)
  constexpr int ESZ = F32 ? 4 : 2;
  constexpr int QL = F32 ? 16 : 8;                 // 16-byte loads per 64-dim row
  const char* qb = reinterpret_cast<const char*>(p.q);
  const char* kb = reinterpret_cast<const char*>(p.k);
  const char* vb = reinterpret_cast<const char*>(p.v);
  const size_t qoff = ((((size_t)bs * p.Tq_cap + q_t0) * p.N + n) * p.row_pitch_q + h * HD) * ESZ;

  // ---- issue: q (same 128 / 256 bytes for every lane), this lane's key rows, this lane's V chunks -------------------
  u32x4_t qv[QL], kv[KP][QL], vv[KP][8][F32 ? 2 : 1];
#pragma unroll
  for (int c = 0; c < QL; ++c) qv[c] = *reinterpret_cast<const u32x4_t*>(qb + qoff + c * 16);
#pragma unroll
  for (int kp = 0; kp < KP; ++kp) {
    int key = kp * 64 + lane;
    key = key < Tk ? key : Tk - 1;                 // clamped rows are masked below
    const size_t off = ((((size_t)bs * p.Tcap + key) * p.N + n) * p.row_pitch_kv + h * HD) * ESZ;
#pragma unroll
    for (int c = 0; c < QL; ++c) kv[kp][c] = *reinterpret_cast<const u32x4_t*>(kb + off + c * 16);
  }
  const int tsub = lane >> 3, ch = lane & 7;       // P V layout: key = 8 i + tsub, d = 8 ch .. 8 ch + 7
  // fp32 rows with four key passes (the pooling head of the accurate mode: 196 keys): K alone is 256 VGPRs per lane, so the
  // V chunks are requested after the scores have consumed the K rows (two latencies per task instead of 100 spilled VGPRs)
  constexpr bool V_LATE = F32 && KP >= 4;
  auto load_v = [&]() {
#pragma unroll
    for (int kp = 0; kp < KP; ++kp)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        int key = kp * 64 + i * 8 + tsub;
        key = key < Tk ? key : Tk - 1;
        const size_t off = ((((size_t)bs * p.Tcap + key) * p.N + n) * p.row_pitch_kv + h * HD + ch * 8) * ESZ;
        vv[kp][i][0] = *reinterpret_cast<const u32x4_t*>(vb + off);
        if (F32) vv[kp][i][F32 ? 1 : 0] = *reinterpret_cast<const u32x4_t*>(vb + off + 16);
      }
  };
  if (!V_LATE) load_v();
  __builtin_amdgcn_sched_barrier(0);     // keep every load of the task ahead of the arithmetic (one latency per task)

  // ---- scores -----------------------------------------------------------------------------------------------------
  const int qpos = t_past;                         // absolute frame index of the one query
  float sc[KP];
  float mx = -INFINITY;
#pragma unroll
  for (int kp = 0; kp < KP; ++kp) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int c = 0; c < QL; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (F32) {
          a0 = fmaf(__uint_as_float(qv[c][j]), __uint_as_float(kv[kp][c][j]), a0);
        } else {
          a0 = fmaf(bf2f(qv[c][j] & 0xffffu), bf2f(kv[kp][c][j] & 0xffffu), a0);
          a1 = fmaf(__uint_as_float(qv[c][j] & 0xffff0000u), __uint_as_float(kv[kp][c][j] & 0xffff0000u), a1);
        }
      }
    }
    const int key = kp * 64 + lane;
    const bool ok = key < Tk && (!p.causal || key <= qpos);
    sc[kp] = ok ? (a0 + a1) : -INFINITY;
    mx = fmaxf(mx, sc[kp]);
  }
  if (V_LATE) {
    __builtin_amdgcn_sched_barrier(0);
    load_v();
    __builtin_amdgcn_sched_barrier(0);
  }
  mx = wave_max(mx);
  const float c2 = p.scale * 1.44269504088896340736f;
  float pr[KP], sum = 0.f;
#pragma unroll
  for (int kp = 0; kp < KP; ++kp) {
    const float a = (sc[kp] - mx) * c2;
    pr[kp] = __builtin_amdgcn_exp2f(a);       // masked: 2^-inf = 0
    sum += pr[kp];
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;

  // ---- P V ----------------------------------------------------------------------------------------------------------
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
  for (int kp = 0; kp < KP; ++kp)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float pt = __shfl(pr[kp], i * 8 + tsub, 64);          // probability of key kp*64 + 8 i + tsub
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (F32) {
          o[j] = fmaf(pt, __uint_as_float(vv[kp][i][0][j]), o[j]);
          o[4 + j] = fmaf(pt, __uint_as_float(vv[kp][i][F32 ? 1 : 0][j]), o[4 + j]);
        } else {
          o[2 * j] = fmaf(pt, bf2f(vv[kp][i][0][j] & 0xffffu), o[2 * j]);
          o[2 * j + 1] = fmaf(pt, __uint_as_float(vv[kp][i][0][j] & 0xffff0000u), o[2 * j + 1]);
        }
      }
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o[j] += __shfl_xor(o[j], 8, 64);
    o[j] += __shfl_xor(o[j], 16, 64);
    o[j] += __shfl_xor(o[j], 32, 64);
  }
  if (tsub == 0) {
    const size_t o_off = (((size_t)b * p.Tq) * p.N + n) * p.D + h * HD + ch * 8;
    unsigned int hb[8], lb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf(o[j] * inv, hb[j], lb[j]);
    *reinterpret_cast<u32x4_t*>(p.ctx_hi + o_off) = pack_bf8(hb);
    if (F32 || p.ctx_lo) *reinterpret_cast<u32x4_t*>(p.ctx_lo + o_off) = pack_bf8(lb);
  }
}

// The same problem with whole cache lines per load instruction (bf16 rows, <= 128 keys).  A key row of one head is ONE 128-byte
// line; in the kernel above a lane owns a key, so every K load instruction touches 64 lines for 16 bytes each (and is issued
// eight times over the same lines): the vector-memory path serves 8x the lines the data needs.  Here lane = (key mod 8, 16-byte
// chunk) for K exactly as for V: an instruction reads 8 keys x 128 B; the lane dots its 8 dims with its 16 bytes of q (one
// load instead of eight), the 8 chunks of a key meet by three DPP adds (quad_perm x 2, row_half_mirror: bit-identical in all 8
// lanes), so the lane that holds V[key][chunk] already holds p[key] (no ds_bpermute for the probabilities); max / sum / output
// cross the 8 key groups by one DPP row rotate + two xor-shuffles instead of six dependent shuffles each.
template <int CTRL>
SF_DEVICE float dpp_move(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int KP>
__global__ __launch_bounds__(256) void sf_temporal_decode_lines_kernel(SfAttnArgs p, int ntasks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int task = blockIdx.x * 4 + wave;
  if (task >= ntasks) return;
  const int h = task % p.heads, bn = task / p.heads;
  const int b = bn / p.N, n = bn % p.N;
  int q_t0 = p.q_t0, Tk = p.Tk, t_past = p.t_past, bs = b;
  if (p.tab) {                                     // ragged call: this sequence's own {slab, slot, keys}
    const SfStreamSlot e = p.tab[b];
    bs = e.stream; q_t0 = e.slot;
    Tk = min(e.tk, KP * 64);
    t_past = Tk - 1;
  } else if (p.pos_dev) {                                 // streamed frame replayed from the position-free graph: {slot, keys} in one scalar load
    struct __attribute__((aligned(4))) SlotKeys { int slot, tk; };
    const SlotKeys sk = *reinterpret_cast<const SlotKeys*>(p.pos_dev);
    q_t0 = sk.slot;
    Tk = min(sk.tk, KP * 64);
    t_past = Tk - 1;
  }
  const int tsub = lane >> 3, ch = lane & 7;       // key = 64 kp + 8 i + tsub, dims 8 ch .. 8 ch + 7
  const char* kb = reinterpret_cast<const char*>(p.k);
  const char* vb = reinterpret_cast<const char*>(p.v);
  const size_t qoff = ((((size_t)bs * p.Tq_cap + q_t0) * p.N + n) * p.row_pitch_q + h * HD + ch * 8) * 2;
  const u32x4_t qv = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(p.q) + qoff);
  u32x4_t kv[KP][8], vv[KP][8];
#pragma unroll
  for (int kp = 0; kp < KP; ++kp)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int key = kp * 64 + i * 8 + tsub;
      key = key < Tk ? key : Tk - 1;               // clamped rows (one line, already in the cache) are masked below
      const size_t off = ((((size_t)bs * p.Tcap + key) * p.N + n) * p.row_pitch_kv + h * HD + ch * 8) * 2;
      kv[kp][i] = *reinterpret_cast<const u32x4_t*>(kb + off);
      vv[kp][i] = *reinterpret_cast<const u32x4_t*>(vb + off);
    }
  __builtin_amdgcn_sched_barrier(0);     // every load of the task ahead of the arithmetic (one latency per task)

  float qf[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    qf[2 * j] = bf2f(qv[j] & 0xffffu);
    qf[2 * j + 1] = __uint_as_float(qv[j] & 0xffff0000u);
  }
  float sc[KP][8];
  float mx = -INFINITY;
#pragma unroll
  for (int kp = 0; kp < KP; ++kp)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a0 = fmaf(qf[2 * j], bf2f(kv[kp][i][j] & 0xffffu), a0);
        a1 = fmaf(qf[2 * j + 1], __uint_as_float(kv[kp][i][j] & 0xffff0000u), a1);
      }
      float a = a0 + a1;
      a += dpp_move<0xB1>(a);                      // quad_perm [1,0,3,2]
      a += dpp_move<0x4E>(a);                      // quad_perm [2,3,0,1]
      a += dpp_move<0x141>(a);                     // row_half_mirror: the other quad of the 8 chunk lanes
      const int key = kp * 64 + i * 8 + tsub;
      const bool ok = key < Tk && (!p.causal || key <= t_past);
      sc[kp][i] = ok ? a : -INFINITY;
      mx = fmaxf(mx, sc[kp][i]);
    }
  mx = fmaxf(mx, dpp_move<0x128>(mx));             // row_ror:8 : key group tsub ^ 1
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float c2 = p.scale * 1.44269504088896340736f;
  float sum = 0.f;
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
  for (int kp = 0; kp < KP; ++kp)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float pt = __builtin_amdgcn_exp2f((sc[kp][i] - mx) * c2);        // masked: 2^-inf = 0
      sum += pt;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[2 * j] = fmaf(pt, bf2f(vv[kp][i][j] & 0xffffu), o[2 * j]);
        o[2 * j + 1] = fmaf(pt, __uint_as_float(vv[kp][i][j] & 0xffff0000u), o[2 * j + 1]);
      }
    }
  sum += dpp_move<0x128>(sum);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] += dpp_move<0x128>(o[j]);
  sum += __shfl_xor(sum, 16, 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] += __shfl_xor(o[j], 16, 64);
  sum += __shfl_xor(sum, 32, 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] += __shfl_xor(o[j], 32, 64);
  if (tsub == 0) {
    const float inv = 1.0f / sum;
    const size_t o_off = (((size_t)b * p.Tq) * p.N + n) * p.D + h * HD + ch * 8;
    unsigned int hb[8], lb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf(o[j] * inv, hb[j], lb[j]);
    *reinterpret_cast<u32x4_t*>(p.ctx_hi + o_off) = pack_bf8(hb);
    if (p.ctx_lo) *reinterpret_cast<u32x4_t*>(p.ctx_lo + o_off) = pack_bf8(lb);
  }
}
hipError_t sf_launch_temporal_decode(SfTemporalRoute r, const SfAttnArgs& a, hipStream_t s) {
  const int ntasks = a.B * a.N * a.heads;
  const dim3 grid((ntasks + 3) / 4), block(256);
#define SF_TD(F, KPV) return sf_launch(sf_temporal_decode_kernel<F, KPV>, grid, block, 0, s, a, ntasks)
  switch (r) {
    case SF_TROUTE_DECODE_F32_KP1: SF_TD(true, 1);
    case SF_TROUTE_DECODE_F32_KP2: SF_TD(true, 2);
    case SF_TROUTE_DECODE_F32_KP4: SF_TD(true, 4);
    case SF_TROUTE_DECODE_LINES_KP1: return sf_launch(sf_temporal_decode_lines_kernel<1>, grid, block, 0, s, a, ntasks);
    case SF_TROUTE_DECODE_LINES_KP2: return sf_launch(sf_temporal_decode_lines_kernel<2>, grid, block, 0, s, a, ntasks);
    case SF_TROUTE_DECODE_BF16_KP1: SF_TD(false, 1);
    case SF_TROUTE_DECODE_BF16_KP2: SF_TD(false, 2);
    case SF_TROUTE_DECODE_BF16_KP4: SF_TD(false, 4);
    default: return hipErrorInvalidValue;
  }
#undef SF_TD
}
