// Spatial attention, head_dim 64 (gfx950, MFMA 16x16x32 bf16): softmax(q k^T d^-0.5) v over the N patches of one frame
// (reference modeling:688-717).  Three kernels, chosen by sf_spatial_plan() at the end of the file and launched only by
// sf_launch_spatial_plan():
//   sf_spatial_attn_dma_kernel    N <= 224: K / V land in LDS by LDS-DMA as 128-byte-row images (sf_attn_image.h); bf16 rows or
//                                 hi + lo planes (accurate mode), optional dropout, optional compile-time tile count.  Most calls.
//   sf_spatial_attn_kernel        N <= 224, register-staged (round 1): output_attentions, fp32 inputs, the A/B switches.
//   sf_spatial_attn_large_kernel  N > 224: keys stream through LDS in chunks, online softmax.
// (-DSF_LAB adds the persistent kernel of tools/lab/sf_spatial_pers.inc.)
#include "sf_attention_fwd.h"

#define SP_WAVES 8
#define SP_QT 2     // query tiles per wave: 16 * SP_WAVES * SP_QT = 256 >= 224 queries
#define SP_MAX_TILES 14                      // 16-key score tiles a wave of the resident kernels holds in registers
#define SP_MAX_KEYS (16 * SP_MAX_TILES)      // 224: more tokens per frame go to the streaming-key kernel

// ================================================================================================
// Register-staged kernel (round 1): block = (frame, head), 8 waves; K and V^T of the head live in LDS.
// "Swapped" QK^T: the wave computes S^T = K Q^T, so in the MFMA C layout a lane
// holds, for ONE query (column = lane&15), 4 keys per 16-key tile.  The softmax row reduction is
// then in-lane + two xor-shuffles (lanes 16/32 apart), and the exponentiated tile is already in the
// B-operand layout of the second MFMA, O^T = V^T P^T (no LDS round trip for P).  To make the 8
// k-elements a lane feeds to that MFMA contiguous keys, the K rows of each 32-key pair of tiles are
// read in a permuted order (MFMA row i of half hh <-> key 32*kt2 + 8*(i>>2) + 4*hh + (i&3)).
// V is transposed on its way into LDS (V^T[d][key]) so the A-operand is one ds_read_b128.
// ACC = the fp32-accurate mode: fp32 inputs are split into bf16 hi+lo and every product becomes
// hi*hi + hi*lo + lo*hi (same three-term scheme as the GEMM).
// Latency plan: every wave first issues the Q-fragment loads of its (up to two) query tiles, then
// the block stages K / V^T, so the Q latency hides under the staging; the context rows of a query
// tile are staged through a per-wave LDS patch and leave as whole 128-byte rows.
// ================================================================================================

template <bool ACC, int MAXNT2>
__global__ __launch_bounds__(SP_WAVES * 64) void sf_spatial_attn_kernel(SfAttnArgs p, int vpitch, int qsplit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  // qsplit > 1 (few frames in flight, e.g. the per-frame streaming step: 12 (frame, head) problems on 256 CUs): qsplit
  // workgroups per (frame, head); each stages K / V^T (all 8 waves) and then waves 0 .. tpw-1 take one query tile each of
  // the workgroup's share, so qsplit times as many CUs work on the launch
  const int fhq = blockIdx.x / qsplit, qs = blockIdx.x % qsplit;
  const int frame = fhq / p.heads, h = fhq % p.heads;
  const int N = p.N;
  const int nkp = (N + 31) & ~31;
  const int nt2 = nkp >> 5;
  char* k_hi = smem;
  char* k_lo = k_hi + (ACC ? nkp * 128 : 0);
  char* v_hi = k_lo + nkp * 128;
  char* v_lo = v_hi + (ACC ? HD * vpitch : 0);
  char* o_st = v_lo + HD * vpitch + wave * (ACC ? 4096 : 2048);   // per-wave [16 rows][128 B] (hi [, lo])
  const size_t row0 = (size_t)frame * N;
  const int nqt = (N + 15) >> 4;
  const int tpw = (nqt + qsplit - 1) / qsplit;         // query tiles per workgroup when split (<= SP_WAVES)
  auto tile_of = [&](int u) -> int {                     // query tile of this wave in round u, or -1
    if (qsplit == 1) return wave + u * SP_WAVES;
    return (u == 0 && wave < tpw) ? qs * tpw + wave : -1;
  };

  // ---- Q fragments of this wave's query tiles (in flight during the staging below) ----------------
  bf16x8_t qh[SP_QT][2], ql[SP_QT][2];
#pragma unroll
  for (int u = 0; u < SP_QT; ++u) {
    const int qt_u = tile_of(u);
    if (qt_u < 0) continue;
    int qi = qt_u * 16 + l15;
    qi = qi < N ? qi : N - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      load_frag<ACC>(p.q, (row0 + qi) * p.row_pitch_q + h * HD + ks * 32 + g * 8, qh[u][ks], ql[u][ks]);
  }

  // ---- stage K (swizzled rows) -------------------------------------------------------------------
  for (int i = tid; i < nkp * 8; i += SP_WAVES * 64) {
    const int key = i >> 3, c = i & 7;
    u32x4_t hv = {0, 0, 0, 0}, lv = {0, 0, 0, 0};
    if (key < N) {
      bf16x8_t a, b;
      load_frag<ACC>(p.k, (row0 + key) * p.row_pitch_kv + h * HD + c * 8, a, b);
      hv = __builtin_bit_cast(u32x4_t, a);
      lv = __builtin_bit_cast(u32x4_t, b);
    }
    const int off = key * 128 + ((c ^ kswz(key)) << 4);
    *reinterpret_cast<u32x4_t*>(k_hi + off) = hv;
    if (ACC) *reinterpret_cast<u32x4_t*>(k_lo + off) = lv;
  }
  // ---- stage V^T: item = (key pair, 8-wide d chunk) -> 8 dword writes {V[2kp][d], V[2kp+1][d]};
  //      (bank-swizzled, see below) ------------------------------------------------------------------
  for (int i = tid; i < (nkp >> 1) * 8; i += SP_WAVES * 64) {
    const int kp = i >> 3, c = i & 7;
    float v0[8], v1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { v0[j] = 0.f; v1[j] = 0.f; }
    if (2 * kp < N) load8<ACC>(p.v, (row0 + 2 * kp) * p.row_pitch_kv + h * HD + c * 8, v0);
    if (2 * kp + 1 < N) load8<ACC>(p.v, (row0 + 2 * kp + 1) * p.row_pitch_kv + h * HD + c * 8, v1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned int h0, l0, h1, l1;
      split_bf(v0[j], h0, l0);
      split_bf(v1[j], h1, l1);
      // V^T row d = c*8+j, 16-byte key chunks XOR-swizzled by vswz(d): distinct for the 8 rows a wave
      // writes together (d = 8c+j, c = 0..7) AND for the 16 rows one ds_read_b128 group reads
      const int d = c * 8 + j;
      const int off = d * vpitch + ((((kp >> 2) ^ vswz(d)) << 2) + (kp & 3)) * 4;
      *reinterpret_cast<unsigned int*>(v_hi + off) = h0 | (h1 << 16);
      if (ACC) *reinterpret_cast<unsigned int*>(v_lo + off) = l0 | (l1 << 16);
    }
  }
  __syncthreads();

#pragma unroll
  for (int u = 0; u < SP_QT; ++u) {
    const int qt = tile_of(u);
    if (qt < 0 || qt >= nqt) continue;

    // ---- S^T = K Q^T ---------------------------------------------------------------------------
    f32x4_t s[MAXNT2][2];
#pragma unroll
    for (int kt2 = 0; kt2 < MAXNT2; ++kt2) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        if (kt2 < nt2) {
          const int key = kt2 * 32 + (l15 >> 2) * 8 + hh * 4 + (l15 & 3);
          const int sw = kswz(key);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int off = key * 128 + (((ks * 4 + g) ^ sw) << 4);
            const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(k_hi + off);
            if (ACC) {
              const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(k_lo + off);
              acc = mfma16(kl, qh[u][ks], acc);
              acc = mfma16(kh, ql[u][ks], acc);
            }
            acc = mfma16(kh, qh[u][ks], acc);
          }
        }
        s[kt2][hh] = acc;
      }
    }
    // ---- softmax over keys (lane: query l15; keys 32*kt2 + 8*g + 4*hh + r) ------------------------
    float max2;
    const float sum = softmax_tiles<ACC, MAXNT2>(s, nt2, g, p.scale, N >> 5, [&](int, int key) { return key < N; }, &max2);
    const float inv = 1.0f / sum;
    if (p.lse2_out && g == 0) {
      const int qi = qt * 16 + l15;
      if (qi < N) p.lse2_out[((size_t)frame * p.heads + h) * N + qi] = max2 + __log2f(sum);
    }
    if (p.probs) {          // output_attentions: the probabilities leave as fp32 rows (wave-uniform branch)
      const int qi = qt * 16 + l15;
      if (qi < N) {
        float* prow = p.probs + (((size_t)frame * p.heads + h) * N + qi) * N;
#pragma unroll
        for (int kt2 = 0; kt2 < MAXNT2; ++kt2)
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kt2 * 32 + g * 8 + hh * 4 + r;
              if (kt2 < nt2 && key < N) prow[key] = s[kt2][hh][r] * inv;
            }
      }
    }

    // ---- O^T = V^T P^T ----------------------------------------------------------------------------
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
          const int d = dt * 16 + l15;
          const int off = d * vpitch + (((kt2 * 4 + g) ^ vswz(d)) << 4);
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
    // ---- context rows: lane holds d = dt*16 + g*4 .. +4 of query l15 -> per-wave LDS patch -> rows --
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
      const int idx = it * 64 + lane;           // 128 chunks: 16 rows x 8 chunks of 16 B
      const int r = idx >> 3, c = idx & 7;
      const int qi = qt * 16 + r;
      const int off = r * 128 + ((c ^ (r & 7)) << 4);
      if (qi < N) {
        const size_t o_off = (row0 + qi) * p.D + h * HD + c * 8;
        *reinterpret_cast<u32x4_t*>(p.ctx_hi + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + off);
        if (ACC) *reinterpret_cast<u32x4_t*>(p.ctx_lo + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + 2048 + off);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ================================================================================================
// spatial attention, bf16 throughput mode, round 2: the same (frame, head) problem with NO register staging.
//   * K and V go global -> LDS by LDS-DMA (global_load_lds, 16 B per lane, whole 128-byte rows) as plain row-major
//     [key][64] images, 16-byte chunks XOR-swizzled on the SOURCE side (a DMA writes lane-linearly); no VALU, no
//     VGPRs, and the loads of the next workgroup on the CU overlap the arithmetic of this one;
//   * V is never transposed in memory: the A operand of O^T = V^T P^T (lane = head-dim column, k = 8 keys) comes
//     from the row-major image by ds_read_b64_tr_b16 (a 16-lane group reads a [4 x 16] block and receives it transposed);
//     its k order — keys {4g..4g+3} of one 16-key tile and {4g..4g+3} of the next — is exactly how the S^T = K Q^T
//     result tiles sit in the lane (4 consecutive keys per 16-key tile), so K rows are read in NATURAL order and P never
//     touches LDS.  (Round 1 transposed V on its way into LDS with 8 dword writes per item and permuted the K rows:
//     19 of the kernel's 57 us at B = 8 were staging.)
// Used unless the probabilities (output_attentions) or the fp32-accurate mode are requested.
// ================================================================================================
// ACC = the fp32-accurate mode on the same structure: q / k / v arrive as hi + lo bf16 planes (the qkv GEMM writes them
// instead of fp32, same bytes), four images (K hi, V hi, K lo, V lo) land by DMA, every product is three MFMAs
// (lo*hi + hi*lo + hi*hi) and the probabilities are split into hi + lo in registers.
// DROP = dropout on the probabilities (training forward with attention_probs_dropout_prob > 0): its own instance, so that the mask
// arithmetic costs the plain kernel no registers (117 VGPRs = two workgroups per CU; with the branch compiled in: 156, one workgroup)
// NTC = compile-time number of score tiles that hold real keys (13 for the 196 patches of a 224^2 frame), 0 = decided at run time.
// With the count known every `if (tile exists)` of the score / PV loops folds away: hipcc then schedules the 28 K-fragment reads and
// MFMAs of a query tile as ONE block (reads of the next tiles in flight under the MFMAs of this one) instead of fourteen basic blocks
// of [2 ds_read -> wait -> MFMA -> wait -> MFMA] — round 4, found in the ISA, not in a profile.
template <int MAXNT, bool ACC, bool DROP = false, int NTC = 0>       // 16-key tiles held in registers: 14 -> N <= 224
__global__ __launch_bounds__(SP_WAVES * 64) void sf_spatial_attn_dma_kernel(SfAttnArgs p, int qsplit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int fhq = blockIdx.x / qsplit, qs = blockIdx.x % qsplit;
  const int frame = fhq / p.heads, h = fhq % p.heads;
  const int N = p.N;
  const int nkp = NTC ? ((NTC + 1) & ~1) * 16 : (N + 31) & ~31;      // keys padded to whole 32-key pairs of tiles
  const int nt = nkp >> 4;
  char* k_img = smem;
  char* v_img = k_img + nkp * 128;
  char* kl_img = v_img + nkp * 128;                      // ACC only
  char* vl_img = kl_img + nkp * 128;
  char* o_st = v_img + nkp * 128 * (ACC ? 3 : 1) + wave * (ACC ? 4096 : 2048);          // per-wave [16 rows][128 B] (hi [, lo])
  const size_t row0 = (size_t)frame * N;
  const int nqt = (N + 15) >> 4;
  const int tpw = (nqt + qsplit - 1) / qsplit;
  auto tile_of = [&](int u) -> int {
    if (qsplit == 1) return wave + u * SP_WAVES;
    return (u == 0 && wave < tpw) ? qs * tpw + wave : -1;
  };

  // ---- K / V images by LDS-DMA: instruction j covers rows 8j .. 8j+7 (lane -> row 8j + lane/8, slot lane%8) -------------
  const bf16_t* kbase = reinterpret_cast<const bf16_t*>(p.k) + h * HD;
  const bf16_t* vbase = reinterpret_cast<const bf16_t*>(p.v) + h * HD;
  for (int j = wave; j < (nkp >> 3); j += SP_WAVES) {
    const int row = j * 8 + (lane >> 3);
    const int chunk = img_dma_chunk(lane, row);         // the slot this lane fills holds logical chunk `chunk`
    const int key = row < N ? row : N - 1;               // padding rows repeat the last key (masked in the softmax, P = 0 for V)
    const size_t src = (row0 + key) * (size_t)p.row_pitch_kv + chunk * 8;
    __builtin_amdgcn_global_load_lds((dma_gptr_t)(kbase + src), (dma_lptr_t)(k_img + j * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((dma_gptr_t)(vbase + src), (dma_lptr_t)(v_img + j * 1024), 16, 0, 0);
    if (ACC) {
      __builtin_amdgcn_global_load_lds((dma_gptr_t)(kbase + p.lo_plane_off + src), (dma_lptr_t)(kl_img + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((dma_gptr_t)(vbase + p.lo_plane_off + src), (dma_lptr_t)(vl_img + j * 1024), 16, 0, 0);
    }
  }
  // ---- Q fragments of this wave's query tiles (register loads, in flight with the DMA) -------------------------------
  bf16x8_t qh[SP_QT][2], ql[SP_QT][2];
#pragma unroll
  for (int u = 0; u < SP_QT; ++u) {
    const int qt_u = tile_of(u);
    if (qt_u < 0) continue;
    int qi = qt_u * 16 + l15;
    qi = qi < N ? qi : N - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16_t* qp = reinterpret_cast<const bf16_t*>(p.q) + (row0 + qi) * p.row_pitch_q + h * HD + ks * 32 + g * 8;
      qh[u][ks] = *reinterpret_cast<const bf16x8_t*>(qp);
      if (ACC) ql[u][ks] = *reinterpret_cast<const bf16x8_t*>(qp + p.lo_plane_off);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c2 = p.scale * 1.44269504088896340736f;
#pragma unroll
  for (int u = 0; u < SP_QT; ++u) {
    const int qt = tile_of(u);
    if (qt < 0 || qt >= nqt) continue;
    // ---- S^T = K Q^T, natural key order: lane (query l15, g) holds keys 16 jt + 4 g + r ---------------------------------
    f32x4_t s[MAXNT];
#pragma unroll
    for (int jt = 0; jt < MAXNT; ++jt) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      if (NTC ? jt < NTC : jt * 16 < N) {                  // tiles made of padding keys only are never computed
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8_t kh = row_frag(k_img, jt * 16 + l15, ks * 4 + g);
          if (ACC) {
            acc = mfma16(row_frag(kl_img, jt * 16 + l15, ks * 4 + g), qh[u][ks], acc);
            acc = mfma16(kh, ql[u][ks], acc);
          }
          acc = mfma16(kh, qh[u][ks], acc);
        }
      }
      s[jt] = acc;
    }
    // mask + row maximum in a SECOND pass over the finished tiles.  Taking the maximum of a tile right behind its MFMA
    // (v_max on the accumulator VGPRs two instructions after v_mfma_f32_16x16x32_bf16) gave run-to-run different maxima on
    // gfx950 / hipcc 7.2 — the VALU read of a still-in-flight MFMA result; results stayed within tolerance (softmax is
    // shift-invariant) but were not bit-reproducible.  Here every tile is read long after its last MFMA issued.
    __builtin_amdgcn_sched_barrier(0);
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < MAXNT; ++jt) {
      if (NTC ? jt < NTC : jt * 16 < N) {
        if (NTC ? jt == NTC - 1 : jt * 16 + 16 > N) {      // the tile that holds the first padding keys
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (jt * 16 + 4 * g + r >= N) s[jt][r] = -INFINITY;
        }
        mx = fmaxf(mx, fmaxf(fmaxf(s[jt][0], s[jt][1]), fmaxf(s[jt][2], s[jt][3])));
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < MAXNT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = 0.f;
        if (NTC ? jt < NTC : jt * 16 < N) e = __builtin_amdgcn_exp2f(fmaf(s[jt][r], c2, -mc));
        s[jt][r] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if (p.lse2_out && g == 0) {        // training forward: base-2 log-sum-exp of the scaled scores, kept for the backward kernel
      const int qi = qt * 16 + l15;
      if (qi < N) p.lse2_out[((size_t)frame * p.heads + h) * N + qi] = mc + __log2f(sum);
    }
    if (DROP && p.drop.on) {           // training: dropout on the (normalised) probabilities (modeling:705) — `sum` above is unmasked
      const int qd = qt * 16 + l15 < N ? qt * 16 + l15 : N - 1;
      const unsigned dbase = (unsigned)((((size_t)frame * p.heads + h) * N + qd) * N);
#pragma unroll
      for (int jt = 0; jt < MAXNT; ++jt)
        if (NTC ? jt < NTC : jt * 16 < N) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = jt * 16 + 4 * g + r;
            s[jt][r] *= sf_drop_factor(p.drop, dbase + (unsigned)(key < N ? key : N - 1));
          }
        }
    }

    // ---- O^T = V^T P^T: 32 keys per step, V^T fragments by transposed reads of the row-major image ------------------------
    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j2 = 0; j2 < MAXNT / 2; ++j2) {
      if (NTC ? 2 * j2 < ((NTC + 1) & ~1) : 2 * j2 < nt) {
        const u32x4_t pu = {pack_bf2(s[2 * j2][0], s[2 * j2][1]), pack_bf2(s[2 * j2][2], s[2 * j2][3]),
                            pack_bf2(s[2 * j2 + 1][0], s[2 * j2 + 1][1]), pack_bf2(s[2 * j2 + 1][2], s[2 * j2 + 1][3])};
        const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pu);
        bf16x8_t pl;
        if (ACC) {
          u32x4_t lu;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const f32x4_t& sv = s[2 * j2 + (w >> 1)];
            const int r0 = (w & 1) * 2;
            lu[w] = pack_bf2(sv[r0] - bf2f(pu[w] & 0xffffu), sv[r0 + 1] - bf2f(pu[w] >> 16));
          }
          pl = __builtin_bit_cast(bf16x8_t, lu);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8_t vh = tr_frag<true>(v_img, j2 * 32, dt, lane);
          if (ACC) {
            o[dt] = mfma16(tr_frag<true>(vl_img, j2 * 32, dt, lane), pf, o[dt]);
            o[dt] = mfma16(vh, pl, o[dt]);
          }
          o[dt] = mfma16(vh, pf, o[dt]);
        }
      }
    }
    // ---- context rows: lane holds d = dt*16 + g*4 .. +4 of query l15 -> per-wave LDS patch -> whole 128-byte rows ---------
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
      const int qi = qt * 16 + r;
      if (qi < N) {
        const size_t oo = (row0 + qi) * p.D + h * HD + c * 8;
        *reinterpret_cast<u32x4_t*>(p.ctx_hi + oo) = *reinterpret_cast<const u32x4_t*>(o_st + r * 128 + ((c ^ (r & 7)) << 4));
        if (ACC) *reinterpret_cast<u32x4_t*>(p.ctx_lo + oo) = *reinterpret_cast<const u32x4_t*>(o_st + 2048 + r * 128 + ((c ^ (r & 7)) << 4));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

#ifdef SF_LAB      // measured slower than the two-workgroups-per-CU kernel above (profiles/r04_spatial_pers_lab.txt): lab library only, source in tools/lab/
#include "sf_spatial_pers.inc"      // build.py --lab puts tools/lab/ on the include path
#endif   // SF_LAB

// ================================================================================================
// spatial attention for N > 224 tokens per frame (higher-resolution inputs, modeling:380-411 resizes
// the position table): block = (frame, head, block of 128 queries), 8 waves = one 16-query tile each;
// keys stream through LDS in chunks of 128 (K rows + V^T, same images and swizzles as above) with the
// online-softmax recurrence (running max m, running sum l, accumulators rescaled by 2^((m - m')c)).
// The score layout keeps a lane on one query, so the rescale is lane-local.
// ================================================================================================
#define SL_KC 128                 // keys per chunk (= 4 tiles of 32; V^T rows are 256 B = 16 chunks, as vswz wants)

template <bool ACC>
__global__ __launch_bounds__(SP_WAVES * 64) void sf_spatial_attn_large_kernel(SfAttnArgs p, int qblocks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int VP = 2 * SL_KC;   // V^T row pitch in bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int qb = blockIdx.x % qblocks;
  const int fh = blockIdx.x / qblocks;
  const int frame = fh / p.heads, h = fh % p.heads;
  const int N = p.N;
  char* k_hi = smem;
  char* k_lo = k_hi + (ACC ? SL_KC * 128 : 0);
  char* v_hi = k_lo + SL_KC * 128;
  char* v_lo = v_hi + (ACC ? HD * VP : 0);
  char* o_st = v_lo + HD * VP + wave * (ACC ? 4096 : 2048);
  const size_t row0 = (size_t)frame * N;
  const int qt = qb * SP_WAVES + wave;                 // this wave's query tile
  const bool active = qt * 16 < N;

  bf16x8_t qh[2], ql[2];
  {
    int qi = qt * 16 + l15;
    qi = qi < N ? qi : N - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) load_frag<ACC>(p.q, (row0 + qi) * p.row_pitch_q + h * HD + ks * 32 + g * 8, qh[ks], ql[ks]);
  }
  const float c = p.scale * 1.44269504088896340736f;
  float m = -INFINITY, l = 0.f;                        // running max (raw scores) and sum, per query (lane l15, partial over g)
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int key0 = 0; key0 < N; key0 += SL_KC) {
    __syncthreads();                                   // previous chunk fully consumed
    for (int i = tid; i < SL_KC * 8; i += SP_WAVES * 64) {
      const int key = i >> 3, ch = i & 7;
      u32x4_t hv = {0, 0, 0, 0}, lv = {0, 0, 0, 0};
      if (key0 + key < N) {
        bf16x8_t a, b;
        load_frag<ACC>(p.k, (row0 + key0 + key) * p.row_pitch_kv + h * HD + ch * 8, a, b);
        hv = __builtin_bit_cast(u32x4_t, a);
        lv = __builtin_bit_cast(u32x4_t, b);
      }
      const int off = key * 128 + ((ch ^ kswz(key)) << 4);
      *reinterpret_cast<u32x4_t*>(k_hi + off) = hv;
      if (ACC) *reinterpret_cast<u32x4_t*>(k_lo + off) = lv;
    }
    for (int i = tid; i < (SL_KC >> 1) * 8; i += SP_WAVES * 64) {
      const int kp = i >> 3, ch = i & 7;
      float v0[8], v1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v0[j] = 0.f; v1[j] = 0.f; }
      if (key0 + 2 * kp < N) load8<ACC>(p.v, (row0 + key0 + 2 * kp) * p.row_pitch_kv + h * HD + ch * 8, v0);
      if (key0 + 2 * kp + 1 < N) load8<ACC>(p.v, (row0 + key0 + 2 * kp + 1) * p.row_pitch_kv + h * HD + ch * 8, v1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned int h0, l0, h1, l1;
        split_bf(v0[j], h0, l0);
        split_bf(v1[j], h1, l1);
        const int d = ch * 8 + j;
        const int off = d * VP + ((((kp >> 2) ^ vswz(d)) << 2) + (kp & 3)) * 4;
        *reinterpret_cast<unsigned int*>(v_hi + off) = h0 | (h1 << 16);
        if (ACC) *reinterpret_cast<unsigned int*>(v_lo + off) = l0 | (l1 << 16);
      }
    }
    __syncthreads();
    if (!active) continue;                             // wave-uniform; barriers stay outside

    f32x4_t s[4][2];
#pragma unroll
    for (int kt2 = 0; kt2 < 4; ++kt2)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const int key = kt2 * 32 + (l15 >> 2) * 8 + hh * 4 + (l15 & 3);
        const int sw = kswz(key);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int off = key * 128 + (((ks * 4 + g) ^ sw) << 4);
          const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(k_hi + off);
          if (ACC) {
            const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(k_lo + off);
            acc = mfma16(kl, qh[ks], acc);
            acc = mfma16(kh, ql[ks], acc);
          }
          acc = mfma16(kh, qh[ks], acc);
        }
        s[kt2][hh] = acc;
      }
    // lane: query l15; keys key0 + 32*kt2 + 8*g + 4*hh + r
    float cm = -INFINITY;
#pragma unroll
    for (int kt2 = 0; kt2 < 4; ++kt2)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (key0 + kt2 * 32 + g * 8 + hh * 4 + r >= N) s[kt2][hh][r] = -INFINITY;
          cm = fmaxf(cm, s[kt2][hh][r]);
        }
    cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
    cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
    const float mn = fmaxf(m, cm);                     // finite: every chunk holds at least one valid key
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
    const float mc = mn * c;
    float add = 0.f;
#pragma unroll
    for (int kt2 = 0; kt2 < 4; ++kt2)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float a = fmaf(s[kt2][hh][r], c, -mc);
          const float e = __builtin_amdgcn_exp2f(a);
          s[kt2][hh][r] = e;
          add += e;
        }
    l = l * alpha + add;
    m = mn;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
    for (int kt2 = 0; kt2 < 4; ++kt2) {
      bf16x8_t ph, pl;
      pack_p<ACC>(s[kt2][0], s[kt2][1], ph, pl);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int d = dt * 16 + l15;
        const int off = d * VP + (((kt2 * 4 + g) ^ vswz(d)) << 4);
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
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = active ? 1.0f / l : 0.f;
  if (p.probs) {
    // output_attentions above 224 patches (round 4): a second sweep over the keys with the FINAL row maximum and sum — the scores of a
    // chunk are recomputed from the re-staged K rows and leave as probabilities, [frames, heads, N, N] fp32 (modeling:703-716)
    const float mc = m * c;
    for (int key0 = 0; key0 < N; key0 += SL_KC) {
      __syncthreads();
      for (int i = tid; i < SL_KC * 8; i += SP_WAVES * 64) {
        const int key = i >> 3, ch = i & 7;
        u32x4_t hv = {0, 0, 0, 0}, lv = {0, 0, 0, 0};
        if (key0 + key < N) {
          bf16x8_t a, b;
          load_frag<ACC>(p.k, (row0 + key0 + key) * p.row_pitch_kv + h * HD + ch * 8, a, b);
          hv = __builtin_bit_cast(u32x4_t, a);
          lv = __builtin_bit_cast(u32x4_t, b);
        }
        const int off = key * 128 + ((ch ^ kswz(key)) << 4);
        *reinterpret_cast<u32x4_t*>(k_hi + off) = hv;
        if (ACC) *reinterpret_cast<u32x4_t*>(k_lo + off) = lv;
      }
      __syncthreads();
      if (!active) continue;
      const int qi = qt * 16 + l15;
#pragma unroll
      for (int kt2 = 0; kt2 < 4; ++kt2)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
          const int key = kt2 * 32 + (l15 >> 2) * 8 + hh * 4 + (l15 & 3);
          const int sw = kswz(key);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int off = key * 128 + (((ks * 4 + g) ^ sw) << 4);
            const bf16x8_t kh = *reinterpret_cast<const bf16x8_t*>(k_hi + off);
            if (ACC) {
              const bf16x8_t kl = *reinterpret_cast<const bf16x8_t*>(k_lo + off);
              acc = mfma16(kl, qh[ks], acc);
              acc = mfma16(kh, ql[ks], acc);
            }
            acc = mfma16(kh, qh[ks], acc);
          }
          // lane: query l15; keys key0 + 32 kt2 + 8 g + 4 hh + r
          const int kbase = key0 + kt2 * 32 + g * 8 + hh * 4;
          if (qi < N) {
            float* dst = p.probs + (((size_t)frame * p.heads + h) * N + qi) * (size_t)N + kbase;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (kbase + r < N) dst[r] = __builtin_amdgcn_exp2f(fmaf(acc[r], c, -mc)) * inv;
          }
        }
    }
  }
  if (!active) return;
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
    const int r = idx >> 3, ch = idx & 7;
    const int qi = qt * 16 + r;
    const int off = r * 128 + ((ch ^ (r & 7)) << 4);
    if (qi < N) {
      const size_t o_off = (row0 + qi) * p.D + h * HD + ch * 8;
      *reinterpret_cast<u32x4_t*>(p.ctx_hi + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + off);
      if (ACC) *reinterpret_cast<u32x4_t*>(p.ctx_lo + o_off) = *reinterpret_cast<const u32x4_t*>(o_st + 2048 + off);
    }
  }
}

// ================================================================================================
// Which kernel a call runs: decided by sf_spatial_plan (no launch), launched by sf_launch_spatial_plan (nothing else names a
// spatial kernel instance).  sf_op_spatial_attention_plan reports the plan; tests/test_hip_parity.py pins it.
// ================================================================================================
static int sp_staged_vpitch(int nkp) { return (2 * nkp + 255) & ~255; }      // V^T row pitch of the staged kernel: whole groups of 16 chunks (vswz is 4-bit)
#ifdef SF_LAB
static int sp_cus() { const int cus = sf_device_cus(); return cus > 0 ? cus : 256; }
#endif

SfSpatialPlan sf_spatial_plan(const SfAttnArgs& a, bool accurate) {
  const SfSpatialPlan none = {SF_SROUTE_NONE, 0, 0};
  if (a.head_dim && a.head_dim != HD) return {SF_SROUTE_GENERIC, 0, 0};      // sf_attention_generic.hip makes its own checks
  if (a.D != a.heads * HD || a.N <= 0 || a.frames <= 0) return none;
  const bool dma_off = sf_sw(SW_DISABLE_SPATIAL_DMA) != nullptr;
  const bool aligned = (a.row_pitch_kv % 8) == 0;
  if (a.drop.on && (accurate || a.probs || a.N > SP_MAX_KEYS || dma_off || !aligned)) return none;   // dropout: DMA kernel only
  const size_t x2 = accurate ? 2 : 1;
  if (a.N > SP_MAX_KEYS) {                          // streaming-key kernel: one workgroup per block of 16 * SP_WAVES queries
    const int qblocks = (a.N + 16 * SP_WAVES - 1) / (16 * SP_WAVES);
    return {accurate ? SF_SROUTE_LARGE_ACC : SF_SROUTE_LARGE_BF16, qblocks, (size_t)(SL_KC * 128 + HD * 2 * SL_KC + SP_WAVES * 2048) * x2};
  }
  const int nkp = (a.N + 31) & ~31;
  // few (frame, head) problems: split the query tiles of each over several workgroups (each re-stages K / V^T: 50 KB)
  const int nqt = (a.N + 15) >> 4, fh = a.frames * a.heads;
  int qsplit = 1;
  if (!a.probs && a.N > 32) {
    if (fh <= 32) qsplit = (nqt + 1) / 2;           // two query tiles per workgroup: 84 workgroups for one 196-patch frame
    else if (fh <= 64) qsplit = (nqt + 3) / 4;
    else if (fh <= 128) qsplit = (nqt + 7) / 8;
    const char* env = sf_sw(SW_SPATIAL_TPW);   // tuning: query tiles per workgroup
    if (env) qsplit = (nqt + atoi(env) - 1) / atoi(env);
    if (qsplit < 1) qsplit = 1;
  }
  // 193 .. 208 tokens per frame (224^2 inputs): the tile count as a compile-time constant (bit-identical; A/B switch shared by both forms)
  const bool ntc = nqt == SF_SPATIAL_NTC && sf_sw(SW_DISABLE_SPATIAL_NTC) == nullptr;
  if (!accurate && !a.probs && !dma_off && aligned) {
#ifdef SF_LAB
    // many (frame, head) problems: the persistent double-buffered kernel (>= 4 problems per CU, so that the pipeline has something to overlap)
    if (sf_sw(SW_SPATIAL_PERS) && qsplit == 1 && fh >= 4 * sp_cus() && a.N >= 64) return {SF_SROUTE_PERS, 1, (size_t)nkp * 512 + SPP_WAVES * 2048};
#endif
    const size_t lds = (size_t)nkp * 256 + SP_WAVES * 2048;
    return {a.drop.on ? SF_SROUTE_DMA_DROP : ntc ? SF_SROUTE_DMA_BF16_NT13 : SF_SROUTE_DMA_BF16, qsplit, lds};
  }
  if (accurate && !a.in_is_f32) {       // hi + lo bf16 planes (sf_spatial_planes_ok): the DMA kernel with three products
    if (a.probs || a.lo_plane_off <= 0 || !aligned || (a.lo_plane_off % 8)) return none;
    return {ntc ? SF_SROUTE_DMA_PLANES_NT13 : SF_SROUTE_DMA_PLANES, qsplit, (size_t)nkp * 512 + SP_WAVES * 4096};
  }
  return {accurate ? SF_SROUTE_STAGED_ACC : SF_SROUTE_STAGED_BF16, qsplit, (size_t)(nkp * 128 + HD * sp_staged_vpitch(nkp) + SP_WAVES * 2048) * x2};
}

hipError_t sf_launch_spatial_plan(const SfSpatialPlan& pl, const SfAttnArgs& a, hipStream_t s) {
  const dim3 grid(a.frames * a.heads * pl.qsplit), block(SP_WAVES * 64);
  const int vp = sp_staged_vpitch((a.N + 31) & ~31);
#define SF_SD(...) return sf_launch_big_lds(sf_spatial_attn_dma_kernel<SP_MAX_TILES, __VA_ARGS__>, grid, block, pl.lds, s, a, pl.qsplit)
  switch (pl.route) {
    case SF_SROUTE_GENERIC: return sf_launch_attention_generic(a, a.head_dim, false, s);
    case SF_SROUTE_LARGE_BF16: return sf_launch(sf_spatial_attn_large_kernel<false>, grid, block, pl.lds, s, a, pl.qsplit);
    case SF_SROUTE_LARGE_ACC: return sf_launch_big_lds(sf_spatial_attn_large_kernel<true>, grid, block, pl.lds, s, a, pl.qsplit);
    case SF_SROUTE_DMA_BF16: SF_SD(false);
    case SF_SROUTE_DMA_BF16_NT13: SF_SD(false, false, SF_SPATIAL_NTC);
    case SF_SROUTE_DMA_DROP: SF_SD(false, true);
    case SF_SROUTE_DMA_PLANES: SF_SD(true);
    case SF_SROUTE_DMA_PLANES_NT13: SF_SD(true, false, SF_SPATIAL_NTC);
    case SF_SROUTE_STAGED_BF16: return sf_launch_big_lds(sf_spatial_attn_kernel<false, SP_MAX_TILES / 2>, grid, block, pl.lds, s, a, vp, pl.qsplit);
    case SF_SROUTE_STAGED_ACC: return sf_launch_big_lds(sf_spatial_attn_kernel<true, SP_MAX_TILES / 2>, grid, block, pl.lds, s, a, vp, pl.qsplit);
#ifdef SF_LAB
    case SF_SROUTE_PERS: return sf_launch_big_lds(sf_spatial_attn_pers_kernel<SP_MAX_TILES>, dim3(sp_cus()), dim3(SPP_WAVES * 64), pl.lds, s, a, a.frames * a.heads);
#endif
    default: return hipErrorInvalidValue;
  }
#undef SF_SD
}

hipError_t sf_launch_spatial_attention(const SfAttnArgs& a, bool accurate, hipStream_t s) {
  return sf_launch_spatial_plan(sf_spatial_plan(a, accurate), a, s);
}

// accurate mode: may the caller hand q / k / v as hi + lo bf16 planes instead of fp32?  Yes when the plan sends that form to a DMA
// kernel (N and probs are all it looks at there) and the A/B switch that keeps the fp32 path in the tests is not set.
bool sf_spatial_planes_ok(int N, bool probs) {
  static float wanted;                   // a.probs is only ever compared with null by the plan
  SfAttnArgs a = {};
  a.heads = 1; a.D = HD; a.frames = 1; a.N = N; a.lo_plane_off = 8; a.probs = probs ? &wanted : nullptr;
  const SfSpatialRoute r = sf_spatial_plan(a, true).route;
  return !sf_sw(SW_DISABLE_SPATIAL_DMA_ACC) && (r == SF_SROUTE_DMA_PLANES || r == SF_SROUTE_DMA_PLANES_NT13);
}
