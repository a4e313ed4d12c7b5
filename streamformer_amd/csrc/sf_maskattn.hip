// Masked attention, the whole operator: the forward the mask decoder runs (sf_maskdec.hip, through sf_maskattn.h) and trains on
// (streamformer_amd/masked_attention.py), its backward and the mask packer.  The backward keeps nothing of the [F heads, Q, HW]
// probabilities: it recomputes P = exp(scale q.k - stats) and so has to make the forward's scores bit for bit.  Every piece that agreement
// rests on has ONE definition below, used by every kernel that needs it: the float4 type and MFMA wrapper, the eight-chain score tree
// (ma_scores), the visibility of a 16-key tile (ma_tile_vis), the K | V staging (ma_stage_kv), the block decode (ma_query_tile), the
// register column (ma_load_col), the mask row (ma_mask_row), the head-width dispatch (mka_for_width) and the host-side check (mka_check).
//
//   sf_maskdec_attention_kernel   ctx[f, q, h, :] = softmax_j(scale Q . (K_j + kpos_j) | mask[f, q, j]) V_j in fp32 with exact products
//                                 (v_mfma_f32_16x16x4_f32), arithmetic and lane layout of sf_oad_attention_kernel: expf, eight blocked score
//                                 chains, running max / sum over 16-key tiles, zero-staged invisible keys, zeros for a query that sees no
//                                 key.  The mask is bit-packed [F, Q, ceil(HW / 32)] (bit set = key hidden), shared by the heads; a null
//                                 mask is the unmasked Q x Q self-attention.
//                                 WORKGROUP SHAPE: 256 threads = 4 waves on ONE 16-query tile of one (frame, head); the key tiles are dealt
//                                 round-robin to the waves (tile t -> wave t % 4), each wave keeps its own running max / sum / accumulator
//                                 and its own K | V staging area in LDS, and the four partial results meet in LDS at the end in wave order
//                                 (max, then sum of exp(m_w - max) weighted partials).  The grid is F x heads x ceil(Q / 16) workgroups, so
//                                 F = 1, Q = 100, 8 heads is 56 workgroups x 4 waves = 224 waves: close to one per CU of the 256, where one
//                                 wave per tile (sf_oad's shape) would occupy 56.  More waves per tile would leave 784 / 16 = 49 key tiles
//                                 at fewer than 12 each and a merge as long as the work; splitting the 16 queries would halve the MFMA tile.
//                                 SKIP: a key tile hidden from all 16 queries of the workgroup (mask words all set; keys past HW count as
//                                 hidden) is left out before K or V are loaded.  Run unskipped, such a tile scores -inf everywhere: the
//                                 running max stays, the correction is expf(0) = 1, every weight is 0 and the staged rows are zeros, so the
//                                 accumulators do not change: both paths give the same bits.  One owner per output element, fixed order.
//                                 TRAIN (template flag, sf_op_maskattn_forward only): also stats[f, h, q] = m + log l = the log-sum-exp of
//                                 the scaled scores over the visible keys (+inf for a query without one), and a mask per head; the decoder
//                                 runs the instance without it.
//   The backward, in fp32 with the same exact products, on the visible keys:
//     delta = rowsum(dO o ctx)      dV = P^T dO      dS = P o (dO V^T - delta)      dQ = scale dS K      dK = scale dS^T Q.
//   delta is made by the MFMA tree that makes dP = dO V^T, with ctx rows in V's place: for a query with ONE visible key ctx = v, so
//   dP - delta is exactly 0, as it is in softmax's own backward, and not the rounding of two differently ordered sums.
//   sf_maskattn_dq_kernel    the forward's shape: 256 threads = 4 waves on ONE 16-query tile of one (frame, head), key tiles dealt round-robin
//                            (tile t -> wave t % 4), q and dO of the lane's query in registers, K | V of a tile staged in the wave's own LDS
//                            area, S^T and dP^T by the forward's eight-chain tree, dQ^T += K^T dS^T.  The four partial dQ meet in LDS and are
//                            summed in wave order, then scaled.  LDS: 4 x 2 x 16 x (hd + 4) floats = 66 KB at head width 128.
//   sf_maskattn_dkv_kernel   256 threads = 4 waves, each OWNS one 16-key tile of one (frame, head) (64 consecutive keys per workgroup) with
//                            K and V of the lane's key in registers, and loops over the query tiles of that (frame, head): Q and dO of the
//                            16 queries, and their ctx, are staged once per workgroup (three [16][hd + 4] tiles and stats: 24.8 KB at width 128),
//                            S and dP by the same tree with the operands' roles swapped, dV^T += dO^T P, dK^T += Q^T dS.  Each key row has
//                            one owner and the query tiles come in ascending order: one summation order, no atomics.
//   SKIP: dq leaves out a key tile hidden from all 16 queries of its tile before K or V are loaded, exactly as the forward does.  dkv
//   leaves out a query tile before Q or dO are loaded when none of the workgroup's 64 keys is visible to any of its 16 queries (every
//   wave reads the 32 mask words that decide it, so the decision is uniform without a barrier), and a wave leaves out the arithmetic when
//   its own 16 keys are not.  Run unskipped (no_skip), such a pair has P = 0 and dS = 0 by selection, not by arithmetic, and an
//   accumulator that gets +-0 added keeps its bits (it is never -0: it starts at +0 and a cancelled sum rounds to +0).
//   Bits of keys at or past HW are never looked at: a key index is compared with HW before its bit is used, and the whole-word tests
//   mask the last word.
//   sf_maskattn_pack_kernel  bool [R, Q, HW] -> uint32 [R, Q, ceil(HW / 32)]: one wave per 64 keys of a row, one ballot, two words.
#include "sf_handle.h"
#include "sf_maskattn.h"

#include <initializer_list>

typedef __attribute__((ext_vector_type(4))) float ma4_t;

#define MKA_WAVES 4
#define MKA_MAX_HW (1 << 24)

struct SfMkaBwd : SfMkaCore {
  const float* ctx; const float* stats; const float* d_ctx;      // [F Tq, heads * hd], [F, heads, Tq], [F Tq, heads * hd]
  float* dq; float* dk; float* dv;
  int dq_pitch, dkv_pitch;
};

// ------------------------------------------------------------------------------------------------
// the pieces the forward and the backward share
// ------------------------------------------------------------------------------------------------
SF_DEVICE ma4_t ma_mfma(float a, float b, ma4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

SF_DEVICE const uint32_t* ma_mask_row(const SfMkaCore& p, bool per_head, int f, int h, int q) {
  const size_t row = per_head ? ((size_t)f * p.heads + h) * p.Tq + q : (size_t)f * p.Tq + q;
  return p.mask + row * p.words;
}

// the score tree: rows (A operand, from LDS) x the lane's column (B operand, registers); eight chains
template <int NT>
SF_DEVICE ma4_t ma_scores(const float* rows, const float (&col)[NT * 4], int HDQ) {
  ma4_t part[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) part[j] = (ma4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NT * 4; ++i)
    if (i < HDQ) part[i & 7] = ma_mfma(rows[4 * i], col[i], part[i & 7]);
  return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
}

// the same tree with both operands in LDS
template <int NT>
SF_DEVICE ma4_t ma_scores_lds(const float* rows, const float* col, int HDQ) {
  ma4_t part[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) part[j] = (ma4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NT * 4; ++i)
    if (i < HDQ) part[i & 7] = ma_mfma(rows[4 * i], col[4 * i], part[i & 7]);
  return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
}

// the lane's B operand of a score tree: row points at dim g of the lane's row; k-index (g, i) of the score MFMAs is dim 4 i + g
template <int NT>
SF_DEVICE void ma_load_col(const float* row, int HDQ, float (&col)[NT * 4]) {
#pragma unroll
  for (int i = 0; i < NT * 4; ++i) col[i] = i < HDQ ? row[4 * i] : 0.f;
}

// the workgroup of a query-tile kernel: block (f, h, qt), the lane's query qi and the row it reads
struct MaQueryTile { int qt, h, f, qi, qrow; };
SF_DEVICE MaQueryTile ma_query_tile(const SfMkaCore& p, int l15) {
  MaQueryTile t;
  const int qtiles = (p.Tq + 15) >> 4;
  int b = (int)blockIdx.x;
  t.qt = b % qtiles; b /= qtiles;
  t.h = b % p.heads; t.f = b / p.heads;
  t.qi = t.qt * 16 + l15;
  t.qrow = t.qi < p.Tq ? t.qi : p.Tq - 1;              // lanes past Tq repeat the last query, see no key and store nothing
  return t;
}

// keys k0 .. k0 + 15 as the 16 queries of a tile see them.  vis / any bit j: key k0 + j is visible to this lane's query / to one of the
// 16 queries; active: the tile exists and is not skipped (the same in every lane: the four 16-lane groups hold the same 16 queries)
struct MaTileVis { unsigned vis, any; bool active; };
SF_DEVICE MaTileVis ma_tile_vis(const uint32_t* mrow, int k0, int Tk, bool qvalid, int no_skip) {
  MaTileVis t = {0u, 0u, k0 < Tk};
  if (t.active) {
    const int nk = Tk - k0;
    const unsigned valid = nk >= 16 ? 0xffffu : ((1u << nk) - 1u);
    const unsigned hidden = mrow ? (mrow[k0 >> 5] >> (k0 & 31)) & 0xffffu : 0u;
    t.vis = qvalid ? (~hidden & valid) : 0u;
    unsigned any = t.vis;
    any |= __shfl_xor(any, 1, 64); any |= __shfl_xor(any, 2, 64); any |= __shfl_xor(any, 4, 64); any |= __shfl_xor(any, 8, 64);
    t.any = any;
    if (!no_skip && any == 0u) t.active = false;
  }
  return t;
}

// K (+ kpos, unless null) and V of keys k0 .. k0 + 15 of (f, h) into a wave's [16][hd + 4] areas; a key no query of the tile sees (and a
// row past Tk) is staged as zeros (0 * p stays finite)
SF_DEVICE void ma_stage_kv(const SfMkaCore& p, const float* kpos, int pos_pitch, int f, int h, int k0, unsigned any, int lane, float* kt, float* vt) {
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2;
  const size_t kv0 = (size_t)f * p.Tk;
  for (int c = lane; c < 16 * HDQ; c += 64) {
    const int row = c / HDQ, cc = c - row * HDQ;
    ma4_t kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if ((any >> row) & 1u) {
      const size_t key = kv0 + k0 + row;
      kv = *reinterpret_cast<const ma4_t*>(p.k + key * p.kv_pitch + h * HD + cc * 4);
      vv = *reinterpret_cast<const ma4_t*>(p.v + key * p.kv_pitch + h * HD + cc * 4);
      if (kpos) kv += *reinterpret_cast<const ma4_t*>(kpos + (size_t)(k0 + row) * pos_pitch + h * HD + cc * 4);
    }
    *reinterpret_cast<ma4_t*>(kt + row * LD + cc * 4) = kv;
    *reinterpret_cast<ma4_t*>(vt + row * LD + cc * 4) = vv;
  }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int NT, bool TRAIN>      // NT = ceil(head_dim / 16) <= 8; TRAIN: p.stats and p.mask_per_head are read
__global__ __launch_bounds__(64 * MKA_WAVES) void sf_maskdec_attention_kernel(SfMkaFwd p) {
  extern __shared__ __attribute__((aligned(16))) float ma_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int area = 2 * 16 * LD;                        // floats of a wave's staging area
  float* kt = ma_smem + wave * area;
  float* vt = kt + 16 * LD;
  const MaQueryTile b = ma_query_tile(p, l15);
  const int qt = b.qt, h = b.h, f = b.f;
  float qreg[NT * 4];
  ma_load_col<NT>(p.q + ((size_t)f * Tq + b.qrow) * p.q_pitch + h * HD + g, HDQ, qreg);
  const uint32_t* mrow = p.mask ? ma_mask_row(p, false, f, h, b.qrow) : nullptr;
  if (TRAIN && p.mask && p.mask_per_head) mrow = ma_mask_row(p, true, f, h, b.qrow);
  ma4_t o_acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o_acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int ntiles = (Tk + 15) >> 4, rounds = (ntiles + MKA_WAVES - 1) / MKA_WAVES;
  for (int r = 0; r < rounds; ++r) {                   // every wave runs every round: the barriers below are reached by all of them
    const int k0 = (r * MKA_WAVES + wave) * 16;
    const MaTileVis tv = ma_tile_vis(mrow, k0, Tk, b.qi < Tq, p.no_skip);
    __syncthreads();
    if (tv.active) ma_stage_kv(p, p.kpos, p.pos_pitch, f, h, k0, tv.any, lane, kt, vt);
    __syncthreads();
    if (tv.active) {
      // S^T tile: keys k0 + l15 (A operand) x queries (B operand); lane (query l15, g) receives keys k0 + 4 g + r
      ma4_t s4 = ma_scores<NT>(kt + l15 * LD + g, qreg, HDQ);
      float mx = -INFINITY;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = (tv.vis >> (4 * g + rr)) & 1u;
        s4[rr] = ok ? s4[rr] * p.scale : -INFINITY;
        mx = fmaxf(mx, s4[rr]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float corr = m_new == -INFINITY ? 1.f : expf(m_run - m_new);      // no visible key so far: keep zeros
      float psum = 0.f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        s4[rr] = m_new == -INFINITY ? 0.f : expf(s4[rr] - m_new);
        psum += s4[rr];
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * corr + psum;
      m_run = m_new;
      // O^T += V^T P^T: lane (dim l15 of the 16-dim tile, g) supplies V[k0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        o_acc[t] *= corr;
        const int d = t * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float v = d < HD ? vt[(4 * g + rr) * LD + d] : 0.f;
          o_acc[t] = ma_mfma(v, s4[rr], o_acc[t]);
        }
      }
    }
  }
  // ---- the four waves' partial results meet: each leaves (o [16][HD], m [16], l [16]) in its own staging area ----
  __syncthreads();
  {
    float* po = kt;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = t * 16 + 4 * g;
      if (d < HD) *reinterpret_cast<ma4_t*>(po + l15 * HD + d) = o_acc[t];
    }
    if (g == 0) { po[16 * HD + l15] = m_run; po[16 * HD + 16 + l15] = l_run; }
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < 16 * HDQ; idx += 64 * MKA_WAVES) {
    const int qq = idx / HDQ, d = (idx - qq * HDQ) * 4;
    const int qo = qt * 16 + qq;
    if (qo >= Tq) continue;
    float mw[MKA_WAVES], m_all = -INFINITY;
#pragma unroll
    for (int w = 0; w < MKA_WAVES; ++w) { mw[w] = ma_smem[w * area + 16 * HD + qq]; m_all = fmaxf(m_all, mw[w]); }
    ma4_t o = {0.f, 0.f, 0.f, 0.f};
    float l_all = 0.f;
    if (m_all != -INFINITY) {
#pragma unroll
      for (int w = 0; w < MKA_WAVES; ++w) {              // wave order: one fixed summation order
        const float cf = expf(mw[w] - m_all);           // a wave without a visible key: expf(-inf) = 0
        l_all += cf * ma_smem[w * area + 16 * HD + 16 + qq];
        o += cf * *reinterpret_cast<const ma4_t*>(ma_smem + w * area + qq * HD + d);
      }
    }
    const float inv = l_all > 0.f ? 1.0f / l_all : 0.f;      // no visible key: zeros
    o *= inv;
    const size_t ob = ((size_t)f * Tq + qo) * ((size_t)p.heads * HD) + h * HD + d;
    if (p.ctx) *reinterpret_cast<ma4_t*>(p.ctx + ob) = o;
    if (p.ctx_hi) store_planes4(o, p.ctx_hi, p.ctx_lo, ob);
    // m + log l; +inf for a query without a visible key, so that the backward's exp(s - stats) is 0 for it
    if (TRAIN && p.stats && d == 0) p.stats[((size_t)f * p.heads + h) * Tq + qo] = l_all > 0.f ? m_all + logf(l_all) : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// dQ
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(64 * MKA_WAVES) void sf_maskattn_dq_kernel(SfMkaBwd p) {
  extern __shared__ __attribute__((aligned(16))) float ma_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk, C = p.heads * HD;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int area = 2 * 16 * LD;
  float* kt = ma_smem + wave * area;
  float* vt = kt + 16 * LD;
  const MaQueryTile b = ma_query_tile(p, l15);
  const int qt = b.qt, h = b.h, f = b.f;
  for (int c = (int)threadIdx.x; c < 16 * HDQ; c += 64 * MKA_WAVES) {      // ctx of the 16 queries, for delta: the first wave's area
    const int row = c / HDQ, cc = c - row * HDQ, qo = qt * 16 + row < Tq ? qt * 16 + row : Tq - 1;
    *reinterpret_cast<ma4_t*>(ma_smem + row * LD + cc * 4) = *reinterpret_cast<const ma4_t*>(p.ctx + ((size_t)f * Tq + qo) * C + h * HD + cc * 4);
  }
  float qreg[NT * 4], doreg[NT * 4];
  ma_load_col<NT>(p.q + ((size_t)f * Tq + b.qrow) * p.q_pitch + h * HD + g, HDQ, qreg);
  ma_load_col<NT>(p.d_ctx + ((size_t)f * Tq + b.qrow) * C + h * HD + g, HDQ, doreg);
  const float lse = p.stats[((size_t)f * p.heads + h) * Tq + b.qrow];
  const uint32_t* mrow = p.mask ? ma_mask_row(p, p.mask_per_head, f, h, b.qrow) : nullptr;
  __syncthreads();
  // delta = dO . ctx by the tree that makes dP (ctx rows in V's place): a query with ONE visible key has ctx = v, so dP - delta is
  // exactly 0 there, as it is in softmax's own backward.  The tile is [query 4 g + r][query l15]; the diagonal is wanted.
  float delta;
  {
    const ma4_t dt = ma_scores<NT>(ma_smem + l15 * LD + g, doreg, HDQ);
    const int r = l15 & 3;
    const float mine = r == 0 ? dt[0] : r == 1 ? dt[1] : r == 2 ? dt[2] : dt[3];
    delta = __shfl(mine, (l15 >> 2) * 16 + l15, 64);
  }
  ma4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (Tk + 15) >> 4, rounds = (ntiles + MKA_WAVES - 1) / MKA_WAVES;
  for (int r = 0; r < rounds; ++r) {                   // every wave runs every round: the barriers below are reached by all of them
    const int k0 = (r * MKA_WAVES + wave) * 16;
    const MaTileVis tv = ma_tile_vis(mrow, k0, Tk, b.qi < Tq, p.no_skip);
    __syncthreads();
    if (tv.active) ma_stage_kv(p, nullptr, 0, f, h, k0, tv.any, lane, kt, vt);
    __syncthreads();
    if (tv.active) {
      // S^T and dP^T tiles: keys k0 + l15 (A operand) x queries (B operand); lane (query l15, g) receives keys k0 + 4 g + r
      const ma4_t s4 = ma_scores<NT>(kt + l15 * LD + g, qreg, HDQ);
      const ma4_t dp4 = ma_scores<NT>(vt + l15 * LD + g, doreg, HDQ);
      float ds[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = (tv.vis >> (4 * g + rr)) & 1u;
        ds[rr] = ok ? expf(__fmul_rn(s4[rr], p.scale) - lse) * (dp4[rr] - delta) : 0.f;      // the forward's rounded product
      }
      // dQ^T += K^T dS^T: lane (dim l15 of the 16-dim tile, g) supplies K[k0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int d = t * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float kx = d < HD ? kt[(4 * g + rr) * LD + d] : 0.f;
          acc[t] = ma_mfma(kx, ds[rr], acc[t]);
        }
      }
    }
  }
  // ---- the four waves' partial results meet: each leaves dq [16][HD] in its own staging area ----
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = t * 16 + 4 * g;
    if (d < HD) *reinterpret_cast<ma4_t*>(kt + l15 * HD + d) = acc[t];
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < 16 * HDQ; idx += 64 * MKA_WAVES) {
    const int qq = idx / HDQ, d = (idx - qq * HDQ) * 4;
    const int qo = qt * 16 + qq;
    if (qo >= Tq) continue;
    ma4_t o = *reinterpret_cast<const ma4_t*>(ma_smem + qq * HD + d);
#pragma unroll
    for (int w = 1; w < MKA_WAVES; ++w) o += *reinterpret_cast<const ma4_t*>(ma_smem + w * area + qq * HD + d);      // wave order
    o *= p.scale;
    *reinterpret_cast<ma4_t*>(p.dq + ((size_t)f * Tq + qo) * p.dq_pitch + h * HD + d) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// dK, dV
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(64 * MKA_WAVES) void sf_maskattn_dkv_kernel(SfMkaBwd p) {
  extern __shared__ __attribute__((aligned(16))) float ma_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk, C = p.heads * HD;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  float* qs = ma_smem;                                 // Q of the 16 queries [16][LD]
  float* dos = qs + 16 * LD;                           // dO [16][LD]
  float* cs = dos + 16 * LD;                           // ctx [16][LD]
  float* st = cs + 16 * LD;                            // stats [16]
  const int ntiles = (Tk + 15) >> 4, groups = (ntiles + MKA_WAVES - 1) / MKA_WAVES;
  int b = (int)blockIdx.x;
  const int kg = b % groups; b /= groups;
  const int h = b % p.heads, f = b / p.heads;
  const int kbase = kg * 16 * MKA_WAVES, k0 = kbase + wave * 16;
  const bool own = k0 < Tk;                            // a wave past the last key tile stages and waits with the others, nothing else
  const int ki = k0 + l15;
  const bool kvalid = ki < Tk;
  float kreg[NT * 4], vreg[NT * 4];
  {
    const size_t row = (size_t)f * Tk + (kvalid ? ki : Tk - 1);      // B operand: lane (key l15, g) supplies dim 4 i + g
    ma_load_col<NT>(p.k + row * p.kv_pitch + h * HD + g, HDQ, kreg);
    ma_load_col<NT>(p.v + row * p.kv_pitch + h * HD + g, HDQ, vreg);
  }
  ma4_t dk_acc[NT], dv_acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { dk_acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f}; dv_acc[t] = (ma4_t){0.f, 0.f, 0.f, 0.f}; }
  const int qtiles = (Tq + 15) >> 4;
  for (int qt = 0; qt < qtiles; ++qt) {
    const int q0 = qt * 16;
    // ---- is any of the workgroup's 64 keys visible to any of the 16 queries?  32 words, the same in every wave ----
    if (!p.no_skip && p.mask) {
      unsigned v = 0u;
      const int qo = q0 + l15, w = (kbase >> 5) + (g & 1);
      if (lane < 32 && qo < Tq && w < p.words) {
        const int nk = Tk - w * 32;
        v = ~ma_mask_row(p, p.mask_per_head, f, h, qo)[w] & (nk >= 32 ? 0xffffffffu : ((1u << nk) - 1u));
      }
      if (__ballot(v != 0u) == 0ull) continue;          // uniform over the workgroup: no barrier is passed by a part of it
    }
    // ---- which of the lane's four (query q0 + 4 g + r, key ki) pairs are visible ----
    unsigned vis = 0u;
    if (own && kvalid) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int qo = q0 + 4 * g + rr;
        if (qo < Tq && !(p.mask && ((ma_mask_row(p, p.mask_per_head, f, h, qo)[ki >> 5] >> (ki & 31)) & 1u))) vis |= 1u << rr;
      }
    }
    const bool wave_act = p.no_skip ? own : __ballot(vis != 0u) != 0ull;
    __syncthreads();                                   // the previous query tile has been read
    for (int c = (int)threadIdx.x; c < 16 * HDQ; c += 64 * MKA_WAVES) {
      const int row = c / HDQ, cc = c - row * HDQ;
      ma4_t qv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f}, cv = {0.f, 0.f, 0.f, 0.f};
      if (q0 + row < Tq) {
        qv = *reinterpret_cast<const ma4_t*>(p.q + ((size_t)f * Tq + q0 + row) * p.q_pitch + h * HD + cc * 4);
        dv = *reinterpret_cast<const ma4_t*>(p.d_ctx + ((size_t)f * Tq + q0 + row) * C + h * HD + cc * 4);
        cv = *reinterpret_cast<const ma4_t*>(p.ctx + ((size_t)f * Tq + q0 + row) * C + h * HD + cc * 4);
      }
      *reinterpret_cast<ma4_t*>(qs + row * LD + cc * 4) = qv;
      *reinterpret_cast<ma4_t*>(dos + row * LD + cc * 4) = dv;
      *reinterpret_cast<ma4_t*>(cs + row * LD + cc * 4) = cv;
    }
    if (threadIdx.x < 16) st[threadIdx.x] = q0 + (int)threadIdx.x < Tq ? p.stats[((size_t)f * p.heads + h) * Tq + q0 + threadIdx.x] : INFINITY;
    __syncthreads();
    if (wave_act) {
      // S and dP tiles: queries q0 + l15 (A operand, LDS) x keys (B operand, registers); lane (key l15, g) receives queries q0 + 4 g + r
      const ma4_t s4 = ma_scores<NT>(qs + l15 * LD + g, kreg, HDQ);
      const ma4_t dp4 = ma_scores<NT>(dos + l15 * LD + g, vreg, HDQ);
      // delta as in the dq pass, by dP's tree with ctx rows in V's place: [query 4 g + r][query l15], the diagonal to the lanes that want it
      const ma4_t dt = ma_scores_lds<NT>(dos + l15 * LD + g, cs + l15 * LD + g, HDQ);
      float pr[4], ds[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const bool ok = (vis >> rr) & 1u;
        const float delta = __shfl(dt[rr], 20 * g + rr, 64);      // lane (query 4 g + r, g) holds it in element r
        pr[rr] = ok ? expf(__fmul_rn(s4[rr], p.scale) - st[4 * g + rr]) : 0.f;
        ds[rr] = ok ? pr[rr] * (dp4[rr] - delta) : 0.f;
      }
      // dV^T += dO^T P, dK^T += Q^T dS: lane (dim l15 of the 16-dim tile, g) supplies dO | Q [q0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int d = t * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float dx = d < HD ? dos[(4 * g + rr) * LD + d] : 0.f;
          const float qx = d < HD ? qs[(4 * g + rr) * LD + d] : 0.f;
          dv_acc[t] = ma_mfma(dx, pr[rr], dv_acc[t]);
          dk_acc[t] = ma_mfma(qx, ds[rr], dk_acc[t]);
        }
      }
    }
  }
  if (own && kvalid) {                                 // lane (key l15, g) holds dims 16 t + 4 g .. + 3 of its key
    const size_t ob = ((size_t)f * Tk + ki) * p.dkv_pitch + h * HD;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = t * 16 + 4 * g;
      if (d < HD) {
        *reinterpret_cast<ma4_t*>(p.dk + ob + d) = dk_acc[t] * p.scale;
        *reinterpret_cast<ma4_t*>(p.dv + ob + d) = dv_acc[t];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// fn(std::integral_constant<int, NT>) for NT = ceil(hd / 16), the template argument of the three kernels
template <typename Fn>
static hipError_t mka_for_width(int hd, Fn&& fn) {
  switch ((hd + 15) / 16) {
#define MKA_CASE(E) case E: return fn(std::integral_constant<int, E>());
    MKA_CASE(1) MKA_CASE(2) MKA_CASE(3) MKA_CASE(4) MKA_CASE(5) MKA_CASE(6) MKA_CASE(7) MKA_CASE(8)
#undef MKA_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t mka_launch_forward(const SfMkaFwd& p, hipStream_t s) {
  if (p.F < 1 || p.Tq < 1 || p.Tk < 1 || p.heads < 1) return hipErrorInvalidValue;
  if (p.hd < 8 || p.hd > 128 || p.hd % 8) return hipErrorInvalidValue;
  if (!p.q || !p.k || !p.v || (p.mask && p.words < (p.Tk + 31) / 32)) return hipErrorInvalidValue;
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.kpos | (uintptr_t)p.ctx) & 15) return hipErrorInvalidValue;
  if (((uintptr_t)p.ctx_hi | (uintptr_t)p.ctx_lo) & 7 || (((uintptr_t)p.mask | (uintptr_t)p.stats) & 3)) return hipErrorInvalidValue;
  if ((p.q_pitch | p.kv_pitch | p.pos_pitch) & 3) return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)p.F * p.heads * ((p.Tq + 15) / 16);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = (size_t)MKA_WAVES * 2 * 16 * (p.hd + 4) * sizeof(float);      // 66 KB at head_dim 128
  const dim3 grid((unsigned)blocks), block(64 * MKA_WAVES);
  const bool train = p.stats || p.mask_per_head;
  return mka_for_width(p.hd, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    return train ? sf_launch_big_lds(sf_maskdec_attention_kernel<NT, true>, grid, block, lds, s, p)
                 : sf_launch_big_lds(sf_maskdec_attention_kernel<NT, false>, grid, block, lds, s, p);
  });
}

static hipError_t mka_launch_backward(const SfMkaBwd& p, hipStream_t s) {
  const int64_t dq_blocks = (int64_t)p.F * p.heads * ((p.Tq + 15) / 16);
  const int64_t dkv_blocks = (int64_t)p.F * p.heads * (((p.Tk + 15) / 16 + MKA_WAVES - 1) / MKA_WAVES);
  if (dq_blocks > 0x7fffffff || dkv_blocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t dq_lds = (size_t)MKA_WAVES * 2 * 16 * (p.hd + 4) * sizeof(float);      // 66 KB at head_dim 128
  const size_t dkv_lds = ((size_t)3 * 16 * (p.hd + 4) + 16) * sizeof(float);          // 24.8 KB
  const dim3 block(64 * MKA_WAVES);
  return mka_for_width(p.hd, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const hipError_t e = sf_launch_big_lds(sf_maskattn_dq_kernel<NT>, dim3((unsigned)dq_blocks), block, dq_lds, s, p);
    return e != hipSuccess ? e : sf_launch(sf_maskattn_dkv_kernel<NT>, dim3((unsigned)dkv_blocks), block, dkv_lds, s, p);
  });
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
#define MKA_BAD_PITCH "%s: row pitches must be multiples of 4 and at least heads * head_dim = %d"

// what every entry point asks of its arguments, before any launch: `required` pointers are not null, and they and the `optional` ones
// (null allowed) are 16-byte aligned; every pitch holds a row of heads * head_dim floats and is a multiple of 4
static int mka_check(const char* who, int F, int Q, int HW, int heads, int head_dim, std::initializer_list<int> pitches,
                     std::initializer_list<const void*> required, std::initializer_list<const void*> optional) {
  uintptr_t bits = 0;
  for (const void* ptr : required) {
    if (!ptr) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
    bits |= (uintptr_t)ptr;
  }
  for (const void* ptr : optional) bits |= (uintptr_t)ptr;
  if (F < 1 || F > 65535 || Q < 1 || Q > 65535 || HW < 1 || HW > MKA_MAX_HW || heads < 1 || heads > 65535)
    return sf_set_err(SF_ERR_INVALID, "%s: bad shape F=%d (1..65535) Q=%d (1..65535) HW=%d (1..%d) heads=%d (1..65535)", who, F, Q, HW, MKA_MAX_HW, heads);
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "%s: head_dim must be a multiple of 8 in 8..128", who);
  const int D = heads * head_dim;
  int widest = 0;
  for (int pitch : pitches) {
    if (pitch < D || (pitch & 3)) return sf_set_err(SF_ERR_INVALID, MKA_BAD_PITCH, who, D);
    widest = std::max(widest, pitch);
  }
  if ((int64_t)F * (Q > HW ? Q : HW) * widest > (int64_t)0x7fffffff) return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^31 - 1 elements", who);
  if (bits & 15) return sf_set_err(SF_ERR_INVALID, "%s: buffers must be 16-byte aligned", who);
  return SF_OK;
}

static void mka_fill_core(SfMkaCore* a, const float* q, int q_pitch, const float* k, const float* v, int kv_pitch, const uint32_t* mask, int mask_per_head,
                          int F, int Q, int HW, int heads, int head_dim, int no_skip) {
  a->q = q; a->k = k; a->v = v; a->mask = mask; a->q_pitch = q_pitch; a->kv_pitch = kv_pitch;
  a->F = F; a->Tq = Q; a->Tk = HW; a->heads = heads; a->hd = head_dim; a->words = (HW + 31) / 32; a->no_skip = no_skip ? 1 : 0;
  a->mask_per_head = mask && mask_per_head ? 1 : 0;
  a->scale = 1.0f / sqrtf((float)head_dim);
}

// the forward alone, as the decoder runs it (parity tests)
extern "C" int sf_op_maskdec_attention(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const float* k_pos_dev,
                                       int pos_pitch, const uint32_t* mask_dev, float* ctx_dev, uint16_t* ctx_hi_dev, uint16_t* ctx_lo_dev, int F, int Q,
                                       int HW, int heads, int head_dim, int no_skip, sf_stream stream) {
  const char* who = "sf_op_maskdec_attention";
  if (!ctx_dev && !ctx_hi_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  if (ctx_lo_dev && !ctx_hi_dev) return sf_set_err(SF_ERR_INVALID, "%s: a lo plane needs its hi plane", who);
  SF_TRY(mka_check(who, F, Q, HW, heads, head_dim, {q_pitch, kv_pitch}, {q_dev, k_dev, v_dev}, {k_pos_dev, mask_dev, ctx_dev, ctx_hi_dev, ctx_lo_dev}));
  if ((k_pos_dev && pos_pitch < heads * head_dim) || (pos_pitch & 3)) return sf_set_err(SF_ERR_INVALID, MKA_BAD_PITCH, who, heads * head_dim);
  SfMkaFwd a;
  memset(&a, 0, sizeof(a));
  mka_fill_core(&a, q_dev, q_pitch, k_dev, v_dev, kv_pitch, mask_dev, 0, F, Q, HW, heads, head_dim, no_skip);
  a.kpos = k_pos_dev; a.pos_pitch = k_pos_dev ? pos_pitch : 0;
  a.ctx = ctx_dev; a.ctx_hi = ctx_hi_dev; a.ctx_lo = ctx_lo_dev;
  HIP_TRY(mka_launch_forward(a, (hipStream_t)stream));
  return SF_OK;
}

// The same kernel as the training forward of streamformer_amd/masked_attention.py: the row statistics the backward recomputes the
// probabilities from, and a mask that may differ between the heads.  Without both it is sf_op_maskdec_attention.
extern "C" int sf_op_maskattn_forward(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const uint32_t* mask_dev,
                                      int mask_per_head, float* ctx_dev, float* stats_dev, int F, int Q, int HW, int heads, int head_dim, int no_skip,
                                      sf_stream stream) {
  SF_TRY(mka_check("sf_op_maskattn_forward", F, Q, HW, heads, head_dim, {q_pitch, kv_pitch}, {q_dev, k_dev, v_dev, ctx_dev}, {mask_dev, stats_dev}));
  SfMkaFwd a;
  memset(&a, 0, sizeof(a));
  mka_fill_core(&a, q_dev, q_pitch, k_dev, v_dev, kv_pitch, mask_dev, mask_per_head, F, Q, HW, heads, head_dim, no_skip);
  a.ctx = ctx_dev; a.stats = stats_dev;
  HIP_TRY(mka_launch_forward(a, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_maskattn_backward(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const uint32_t* mask_dev,
                                       int mask_per_head, const float* ctx_dev, const float* stats_dev, const float* d_ctx_dev, float* dq_dev,
                                       int dq_pitch, float* dk_dev, float* dv_dev, int dkv_pitch, int F, int Q, int HW, int heads, int head_dim,
                                       int no_skip, sf_stream stream) {
  SF_TRY(mka_check("sf_op_maskattn_backward", F, Q, HW, heads, head_dim, {q_pitch, kv_pitch, dq_pitch, dkv_pitch},
                   {q_dev, k_dev, v_dev, ctx_dev, stats_dev, d_ctx_dev, dq_dev, dk_dev, dv_dev}, {mask_dev}));
  SfMkaBwd a;
  memset(&a, 0, sizeof(a));
  mka_fill_core(&a, q_dev, q_pitch, k_dev, v_dev, kv_pitch, mask_dev, mask_per_head, F, Q, HW, heads, head_dim, no_skip);
  a.ctx = ctx_dev; a.stats = stats_dev; a.d_ctx = d_ctx_dev; a.dq = dq_dev; a.dk = dk_dev; a.dv = dv_dev;
  a.dq_pitch = dq_pitch; a.dkv_pitch = dkv_pitch;
  HIP_TRY(mka_launch_backward(a, (hipStream_t)stream));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// bool mask -> packed words
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_maskattn_pack_kernel(const uint8_t* in, uint32_t* out, long long rows, int HW, int words) {
  const int lane = (int)threadIdx.x & 63, chunks = (HW + 63) >> 6;
  const long long units = rows * chunks, step = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long u = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < units; u += step) {
    const long long row = u / chunks;
    const int ch = (int)(u - row * chunks), key = ch * 64 + lane;
    const bool hidden = key >= HW || in[row * HW + key] != 0;      // padding bits are set
    const unsigned long long bits = __ballot(hidden);
    if (lane < 2 && 2 * ch + lane < words) out[row * words + 2 * ch + lane] = (uint32_t)(bits >> (32 * lane));
  }
}

extern "C" int sf_op_maskattn_pack(const uint8_t* mask_dev, uint32_t* bits_dev, long long rows, int HW, sf_stream stream) {
  const char* who = "sf_op_maskattn_pack";
  if (!mask_dev || !bits_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (rows < 1 || HW < 1 || HW > MKA_MAX_HW) return sf_set_err(SF_ERR_INVALID, "%s: bad shape rows=%lld HW=%d (1..%d)", who, rows, HW, MKA_MAX_HW);
  if ((uintptr_t)bits_dev & 3) return sf_set_err(SF_ERR_INVALID, "%s: bits_dev must be 4-byte aligned", who);
  const int words = (HW + 31) / 32;
  if (rows > 0x7fffffffLL * 32 / HW) return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^36 mask elements", who);
  const long long units = rows * ((HW + 63) / 64);
  const long long grid = std::min<long long>((units + 3) / 4, 65536);
  HIP_TRY(sf_launch(sf_maskattn_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, mask_dev, bits_dev, rows, HW, words));
  return SF_OK;
}
